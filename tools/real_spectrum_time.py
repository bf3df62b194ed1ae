"""Timing of the spectrum of real samples (wr_spectrum_create_real) against what a caller had to do before it: the IQ
spectrum of the same samples with zeros interleaved for Q (development aid; bench.py is the contract).
profiles/real_spectrum.txt was taken with it.

  python tools/real_spectrum_time.py [--windows 8] [--seconds 0.2] [--sizes 1024,4096,65536,1048576]

One process, one device.  Per size: a batch of frames back to back in device memory (256 rows for the sizes of a tuner's
receivers, else as many as --mbytes of real input hold), wr_spectrum_batch_db on a real spectrum and on an IQ spectrum,
the two ALTERNATING window by window; a window repeats the batch until it fills --seconds, between two device events.
The first pair of figures per size is the IQ path against itself (two spectra of the same kind, alternating): the spread
below which a difference means nothing.  Prints one JSON line per size."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=8)
ap.add_argument("--seconds", type=float, default=0.2)
ap.add_argument("--sizes", default="1024,4096,65536,1048576")
ap.add_argument("--mbytes", type=int, default=64, help="real input per batch of the large sizes")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch                                              # noqa: E402
from webradio_amd.device import Device, Spectrum          # noqa: E402

dev = Device(0, torch.cuda.current_stream().cuda_stream)


def ms_per_batch(spec, x, rows, out, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        spec.batch_db(x, rows, out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reps_for(spec, x, rows, out):
    for _ in range(3):                                    # warm-up of this shape: code objects, the work area's growth
        spec.batch_db(x, rows, out)
    torch.cuda.synchronize()
    ms = ms_per_batch(spec, x, rows, out, 20)
    return max(8, int(args.seconds * 1e3 / ms) + 1)


def summary(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


for n in (int(s) for s in args.sizes.split(",")):
    rows = 256 if n <= 16384 else max(4, (args.mbytes << 20) // (4 * n))
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    x = torch.randn(rows * n, device="cuda", generator=g) * 0.1
    t = torch.arange(rows * n, device="cuda", dtype=torch.float32)
    x += 0.3 * torch.cos(t * 0.37)
    iq = torch.zeros(2 * rows * n, device="cuda")
    iq[0::2] = x                                          # what a caller did before: zeros for Q, twice the bytes
    out = [torch.empty(rows * n, device="cuda") for _ in range(2)]
    real, cplx, cplx2 = Spectrum(dev, n, real=True), Spectrum(dev, n), Spectrum(dev, n)
    rr, rc = reps_for(real, x, rows, out[0]), reps_for(cplx, iq, rows, out[1])
    reps_for(cplx2, iq, rows, out[1])
    same = float((out[0] - out[1]).abs().max())           # (dB rows of the two paths, everywhere: noise-floor bins included)
    a, b, r, c = [], [], [], []
    for _ in range(args.windows):                         # the same code against itself
        a.append(ms_per_batch(cplx, iq, rows, out[1], rc))
        b.append(ms_per_batch(cplx2, iq, rows, out[1], rc))
    for _ in range(args.windows):                         # real against IQ with zeros
        r.append(ms_per_batch(real, x, rows, out[0], rr))
        c.append(ms_per_batch(cplx, iq, rows, out[1], rc))
    spread = max(abs(u / v - 1.0) for u, v in zip(a, b))
    print(json.dumps({"fft_size": n, "rows": rows, "windows": args.windows, "reps_per_window": {"real": rr, "iq": rc},
                      "iq_ms_per_batch_a": summary(a), "iq_ms_per_batch_b": summary(b),
                      "spread_same_code": round(spread, 4),
                      "real_ms_per_batch": summary(r), "iq_zero_q_ms_per_batch": summary(c),
                      "real_over_iq": round(statistics.median(r) / statistics.median(c), 4),
                      "max_db_difference_real_vs_iq": round(same, 5)}), flush=True)
    for s in (real, cplx, cplx2):
        s.destroy()
    del x, iq, out, t
    torch.cuda.empty_cache()
dev.close()
