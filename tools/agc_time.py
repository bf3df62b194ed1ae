"""Timing of the audio AGC -- k_agc_rows behind a tuner's post stage, and wr_agc_rows on a plain block -- against the same
submit without it and against a plain copy of the same bytes (development aid; bench.py is the contract).
profiles/agc.txt is where its figures go.

  python tools/agc_time.py [--windows 8] [--seconds 0.2]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, blocks of 4 000 000 frames, 2 000 audio
frames per receiver and block (2.05 MB of audio), streaming off in both tuners.  Figures, all between two device events
over repeated calls, ALTERNATING window by window:
  submit_agc    one wr_tuner_submit of a device block with AGC on every receiver: DDC launch, post stage, k_agc_rows;
  submit_plain  the same submit on a twin tuner with no AGC (its post stage rides in the next block's launch);
  submit_plain_b  the same again: the spread below which a difference means nothing;
  rows_256      one wr_agc_rows call on 256 x 2 000 frames.  The call is synchronous -- two small copies in, the kernel, one
                copy out and the wait -- so the figure is the whole call as a caller pays it, not the kernel alone (that: a
                rocprofv3 --kernel-trace --stats run of this tool);
  rows_64       the same on 64 x 2 000: a quarter of the workgroups, three quarters of the CUs idle;
  copy          a device-to-device copy of the same 2.05 MB: the price of touching those bytes once.
Prints one JSON line."""
import json
import statistics

import timing

args = timing.parse(timing.parser())

import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402
from webradio_amd import synth                            # noqa: E402
from webradio_amd.device import agc_design                # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K2 = NFRAMES // (C2["input_rate"] // C2["audio_rate"])
BYTES = K2 * NRX * 4

dev, ifs, block = timing.c2_case()
with_agc, plain = timing.c2_tuner(dev, ifs, agc=True)[0], timing.c2_tuner(dev, ifs)[0]
rows = torch.randn(NRX * K2, device="cuda")
target, floor_bits, step = agc_design(audio_rate=C2["audio_rate"])
par = {n: (np.full(n, target, np.float32), np.full(n, floor_bits, np.uint32), np.full(n, step, np.uint32)) for n in (NRX, 64)}


def submit_agc():
    with_agc.submit_device(block, NFRAMES)


def submit_plain():
    plain.submit_device(block, NFRAMES)


def rows_n(n):
    t, f, s = par[n]
    return lambda: dev.agc_rows(rows.data_ptr(), K2, n, K2, t, f, s, f)


fns = {"submit_agc": submit_agc, "submit_plain": submit_plain, "submit_plain_b": submit_plain, "rows_256": rows_n(NRX),
       "rows_64": rows_n(64), "copy": timing.copier(BYTES)}
got, reps = timing.measure(fns, args)
with_agc.flush()
plain.flush()
torch.cuda.synchronize()
on, launches = with_agc.agc_info()
assert on == NRX and launches > 0 and plain.agc_info() == (0, 0)
med = {k: statistics.median(v) for k, v in got.items()}
print(json.dumps({"receivers": NRX, "k2": K2, "bytes": BYTES, "step": step, "windows": args.windows, "reps_per_window": reps,
                  **{k + "_us": timing.summary(v) for k, v in got.items()},
                  "spread_same_code": timing.spread(got["submit_plain"], got["submit_plain_b"]),
                  "agc_in_a_submit_us": round(med["submit_agc"] - 0.5 * (med["submit_plain"] + med["submit_plain_b"]), 2),
                  "rows_64_over_rows_256": round(med["rows_64"] / med["rows_256"], 3),
                  "rows_256_over_copy": round(med["rows_256"] / med["copy"], 3)}), flush=True)
with_agc.destroy()
plain.destroy()
dev.close()
