"""Timing of the tone bank -- wr_tones_push_rows on a plain block of rows, and wr_tuner_tones_push behind a submit -- against
the same submit without it and against a plain copy of the same bytes (development aid; bench.py is the contract).
profiles/tones.txt is where its figures go.

  python tools/tones_time.py [--windows 8] [--seconds 0.2]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, blocks of 4 000 000 frames, 2 000 audio
frames per receiver and block (2.05 MB of audio), the 50 CTCSS tones, a window of 12 500 frames (0.25 s at 50 kHz),
streaming off in both tuners.  Figures, all between two device events over repeated calls, ALTERNATING window by window:
  rows_256       one wr_tones_push_rows call on 256 x 2 000 frames (asynchronous: k_tones_part and k_tones_latch, no copy);
  rows_64        the same on 64 x 2 000: a quarter of the workgroups;
  submit_push    one wr_tuner_submit of a device block followed by wr_tuner_tones_push: DDC launch, the post stage on its
                 own (the push wants the block's audio now, so it cannot ride in the next block's launch), the two kernels;
  submit_flush   the same submit followed by wr_tuner_flush on a twin tuner: what any getter of the block's audio costs;
  submit_plain   the same submit alone on a third twin (its post stage rides in the next block's launch);
  submit_plain_b the same again: the spread below which a difference means nothing;
  copy           a device-to-device copy of the same 2.05 MB: the price of touching those bytes once.
Prints one JSON line."""
import json

import timing

args = timing.parse(timing.parser())

import torch                                              # noqa: E402
from webradio_amd import CTCSS_HZ, synth                  # noqa: E402
from webradio_amd.device import ToneBank                  # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K2 = NFRAMES // (C2["input_rate"] // C2["audio_rate"])
WINDOW = 12_500

dev, ifs, block = timing.c2_case()
bank = ToneBank(dev, NRX, CTCSS_HZ, C2["audio_rate"], WINDOW)
rows_bank = ToneBank(dev, NRX, CTCSS_HZ, C2["audio_rate"], WINDOW)
rows = 0.05 * torch.randn(NRX * K2, device="cuda")

figures = timing.row_bank_figures(args, dev, ifs, block, lambda tuner: tuner.tones_push(bank),
                                  lambda n: lambda: rows_bank.push_rows(rows.data_ptr(), K2, n, K2), K2 * NRX * 4)
iq, energy, windows, fill = bank.read()
assert int(windows[0]) > 0 and int(energy[0]) > 0 and int(windows[0]) == int(windows[NRX - 1])
print(json.dumps({"receivers": NRX, "k2": K2, "tones": len(CTCSS_HZ), "window": WINDOW, **figures}), flush=True)
bank.destroy()
rows_bank.destroy()
dev.close()
