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
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=8)
ap.add_argument("--seconds", type=float, default=0.2)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch                                               # noqa: E402
from webradio_amd import capi, synth                       # noqa: E402
from webradio_amd.device import Device, Resampler, Tuner   # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K2 = NFRAMES // (C2["input_rate"] // C2["audio_rate"])
BYTES = K2 * NRX * 4
OUT_RATE, TAPS = 48_000, 32

dev = Device(0, torch.cuda.current_stream().cuda_stream)
ifs = synth.c2_ifs()
block = synth.fm_stream_torch(NFRAMES, C2["input_rate"], ifs[::8], "cuda", noise_dbfs=-50.0)


def make():
    t = Tuner(dev, C2["input_rate"], NRX, NFRAMES)
    for f in ifs:
        t.add_receiver(f, C2["chan_passband"], C2["chan_rate"], capi.WR_FM, C2["audio_passband"], C2["audio_rate"])
    return t


pushed, flushed, plain = make(), make(), make()
bank = Resampler(dev, NRX, C2["audio_rate"], OUT_RATE, TAPS)
rows_bank = Resampler(dev, NRX, C2["audio_rate"], OUT_RATE, TAPS)
KOUT = bank.out_frames(K2) + 1                            # (a block yields 1 920 frames at this ratio, whatever the clock)
rows = 0.05 * torch.randn(NRX * K2, device="cuda")
out = torch.empty(NRX * KOUT, device="cuda")
src = torch.randn(BYTES // 4, device="cuda")
dst = torch.empty_like(src)
n_out, slots = capi.C.c_size_t(), capi.C.c_uint()


def us_per_call(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def reps_for(fn):
    for _ in range(3):                                    # warm-up: code objects, uploads
        fn()
    torch.cuda.synchronize()
    return max(8, int(args.seconds * 1e6 / us_per_call(fn, 20)) + 1)


def summary(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def submit_push():
    pushed.submit_device(block, NFRAMES)
    capi.check(dev.lib.wr_tuner_resamp_push(pushed.h, bank.h, capi.ptr(out), KOUT, capi.C.byref(n_out), capi.C.byref(slots)))


def submit_flush():
    flushed.submit_device(block, NFRAMES)
    flushed.flush()


def submit_plain():
    plain.submit_device(block, NFRAMES)


def rows_n(n):
    return lambda: rows_bank.push_rows(rows.data_ptr(), K2, n, K2, out.data_ptr(), KOUT)


def copy():
    dst.copy_(src)


fns = {"rows_256": rows_n(NRX), "rows_64": rows_n(64), "submit_push": submit_push, "submit_flush": submit_flush,
       "submit_plain": submit_plain, "submit_plain_b": submit_plain, "copy": copy}
reps = {k: reps_for(fn) for k, fn in fns.items()}
got = {k: [] for k in fns}
for _ in range(args.windows):
    for k, fn in fns.items():
        got[k].append(us_per_call(fn, reps[k]))
for t in (pushed, flushed, plain):
    t.flush()
torch.cuda.synchronize()
L, M, P, frames_in, frames_out = bank.info()
assert n_out.value == K2 * L // M and slots.value == NRX and frames_in % K2 == 0 and frames_out == frames_in * L // M
assert bool(torch.isfinite(out.view(NRX, KOUT)[:, : n_out.value]).all()) and float(out.abs().max()) > 0
med = {k: statistics.median(v) for k, v in got.items()}
plain_us = 0.5 * (med["submit_plain"] + med["submit_plain_b"])
print(json.dumps({"receivers": NRX, "k2": K2, "L": L, "M": M, "taps_per_phase": P, "out_frames": n_out.value, "bytes": BYTES,
                  "windows": args.windows, "reps_per_window": reps, **{k + "_us": summary(v) for k, v in got.items()},
                  "spread_same_code": round(max(abs(u / v - 1.0) for u, v in zip(got["submit_plain"], got["submit_plain_b"])), 4),
                  "push_in_a_submit_us": round(med["submit_push"] - plain_us, 2),
                  "push_over_a_flush_us": round(med["submit_push"] - med["submit_flush"], 2),
                  "rows_64_over_rows_256": round(med["rows_64"] / med["rows_256"], 3),
                  "rows_256_over_copy": round(med["rows_256"] / med["copy"], 3)}), flush=True)
bank.destroy()
rows_bank.destroy()
for t in (pushed, flushed, plain):
    t.destroy()
dev.close()
