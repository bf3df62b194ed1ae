"""Timing of the DCS bank -- wr_dcs_push_rows on a plain block of rows, and wr_tuner_dcs_push behind a submit -- against the
same submit without it, against the tone bank on the same rows and against a plain copy of the same bytes (development aid;
bench.py is the contract).  profiles/dcs.txt is where its figures go.

  python tools/dcs_time.py [--windows 8] [--seconds 0.2]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, blocks of 4 000 000 frames, 2 000 audio
frames per receiver and block (2.05 MB of audio) at 50 kHz -- 43 chips and five or six evaluations per row and push -- the
104 standard codes, streaming off in both tuners.  Figures, all between two device events over repeated calls, ALTERNATING
window by window:
  rows_256       one wr_dcs_push_rows call on 256 x 2 000 frames (asynchronous: one k_dcs_push launch, no copy);
  rows_64        the same on 64 x 2 000: a quarter of the workgroups;
  submit_push    one wr_tuner_submit of a device block followed by wr_tuner_dcs_push: DDC launch, the post stage on its own
                 (the push wants the block's audio now, so it cannot ride in the next block's launch), the kernel;
  submit_flush   the same submit followed by wr_tuner_flush on a twin tuner: what any getter of the block's audio costs;
  submit_plain   the same submit alone on a third twin (its post stage rides in the next block's launch);
  submit_plain_b the same again: the spread below which a difference means nothing;
  copy           a device-to-device copy of the same 2.05 MB: the price of touching those bytes once;
  tones_rows_256 one wr_tones_push_rows call on the same 256 rows (the 50 CTCSS tones, a window of 12 500 frames).
Prints one JSON line."""
import json

import timing

args = timing.parse(timing.parser())

import torch                                              # noqa: E402
from webradio_amd import CTCSS_HZ, DCS_CODES, synth       # noqa: E402
from webradio_amd.device import DcsBank, ToneBank         # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K2 = NFRAMES // (C2["input_rate"] // C2["audio_rate"])

dev, ifs, block = timing.c2_case()
bank = DcsBank(dev, NRX, DCS_CODES, C2["audio_rate"])
rows_bank = DcsBank(dev, NRX, DCS_CODES, C2["audio_rate"])
tones = ToneBank(dev, NRX, CTCSS_HZ, C2["audio_rate"], 12_500)
rows = 0.05 * torch.randn(NRX * K2, device="cuda")

figures = timing.row_bank_figures(args, dev, ifs, block, lambda tuner: tuner.dcs_push(bank),
                                  lambda n: lambda: rows_bank.push_rows(rows.data_ptr(), K2, n, K2), K2 * NRX * 4,
                                  beside={"tones_rows_256": lambda: tones.push_rows(rows.data_ptr(), K2, NRX, K2)})
agree, run, hits, evals = bank.read()
assert int(evals[0]) > 0 and int(evals[0]) == int(evals[NRX - 1]) == ((bank.info()[3] * bank.step) >> 29) // 8
med = {k: figures[k + "_us"]["median"] for k in ("rows_256", "tones_rows_256")}
print(json.dumps({"receivers": NRX, "k2": K2, "codes": len(DCS_CODES), "step": bank.step, **figures,
                  "rows_256_over_tones_rows_256": round(med["rows_256"] / med["tones_rows_256"], 3)}), flush=True)
bank.destroy()
rows_bank.destroy()
tones.destroy()
dev.close()
