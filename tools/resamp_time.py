"""Timing of the resampler -- wr_resamp_push_rows on a plain block of rows, and wr_tuner_resamp_push behind a submit -- against
the same submit without it and against a plain copy of the same bytes (development aid; bench.py is the contract).
profiles/resamp.txt is where its figures go.

  python tools/resamp_time.py [--windows 8] [--seconds 0.2]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, blocks of 4 000 000 frames, 2 000 audio
frames per receiver and block (2.05 MB of audio) at 50 kHz, resampled to 48 kHz (24 / 25) with 32 taps per phase: 1 920
output frames per receiver and block, streaming off in all tuners.  Figures, all between two device events over repeated
calls, ALTERNATING window by window:
  rows_256       one wr_resamp_push_rows call on 256 x 2 000 frames (asynchronous: k_resamp_rows, no copy);
  rows_64        the same on 64 x 2 000: a quarter of the workgroups (the bank has 256 rows, so the call also clears the
                 histories of the 192 rows it leaves out the first time round);
  submit_push    one wr_tuner_submit of a device block followed by wr_tuner_resamp_push: DDC launch, the post stage on its
                 own (the push wants the block's audio now, so it cannot ride in the next block's launch), the kernel;
  submit_flush   the same submit followed by wr_tuner_flush on a twin tuner: what any getter of the block's audio costs;
  submit_plain   the same submit alone on a third twin (its post stage rides in the next block's launch);
  submit_plain_b the same again: the spread below which a difference means nothing;
  copy           a device-to-device copy of the same 2.05 MB: the price of touching those bytes once.
Prints one JSON line."""
import json

import timing

args = timing.parse(timing.parser())

import torch                                               # noqa: E402
from webradio_amd import capi, synth                       # noqa: E402
from webradio_amd.device import Resampler                  # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K2 = NFRAMES // (C2["input_rate"] // C2["audio_rate"])
OUT_RATE, TAPS = 48_000, 32

dev, ifs, block = timing.c2_case()
bank = Resampler(dev, NRX, C2["audio_rate"], OUT_RATE, TAPS)
rows_bank = Resampler(dev, NRX, C2["audio_rate"], OUT_RATE, TAPS)
KOUT = bank.out_frames(K2) + 1                            # (a block yields 1 920 frames at this ratio, whatever the clock)
rows = 0.05 * torch.randn(NRX * K2, device="cuda")
out = torch.empty(NRX * KOUT, device="cuda")
n_out, slots = capi.C.c_size_t(), capi.C.c_uint()


def push(tuner):
    capi.check(dev.lib.wr_tuner_resamp_push(tuner.h, bank.h, capi.ptr(out), KOUT, capi.C.byref(n_out), capi.C.byref(slots)))


figures = timing.row_bank_figures(args, dev, ifs, block, push,
                                  lambda n: lambda: rows_bank.push_rows(rows.data_ptr(), K2, n, K2, out.data_ptr(), KOUT),
                                  K2 * NRX * 4)
L, M, P, frames_in, frames_out = bank.info()
assert n_out.value == K2 * L // M and slots.value == NRX and frames_in % K2 == 0 and frames_out == frames_in * L // M
assert bool(torch.isfinite(out.view(NRX, KOUT)[:, : n_out.value]).all()) and float(out.abs().max()) > 0
print(json.dumps({"receivers": NRX, "k2": K2, "L": L, "M": M, "taps_per_phase": P, "out_frames": n_out.value, **figures}),
      flush=True)
bank.destroy()
rows_bank.destroy()
dev.close()
