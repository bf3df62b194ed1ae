"""Timing of the spectrum of real samples (wr_spectrum_create_real) against what a caller had to do before it: the IQ
spectrum of the same samples with zeros interleaved for Q (development aid; bench.py is the contract).
profiles/real_spectrum.txt was taken with it.

  python tools/real_spectrum_time.py [--windows 8] [--seconds 0.2] [--sizes 1024,4096,65536,1048576]

One process, one device.  Per size: a batch of frames back to back in device memory (256 rows for the sizes of a tuner's
receivers, else as many as --mbytes of real input hold), wr_spectrum_batch_db on a real spectrum and on an IQ spectrum,
the two ALTERNATING window by window; a window repeats the batch until it fills --seconds, between two device events.
The first pair of figures per size is the IQ path against itself (two spectra of the same kind, alternating): the spread
below which a difference means nothing.  Prints one JSON line per size."""
import json
import statistics

import timing

ap = timing.parser()
ap.add_argument("--sizes", default="1024,4096,65536,1048576")
ap.add_argument("--mbytes", type=int, default=64, help="real input per batch of the large sizes")
args = timing.parse(ap)

import torch                                              # noqa: E402
from webradio_amd.device import Spectrum                  # noqa: E402

dev = timing.open_device()


def summary(ms):
    return timing.summary(ms, 5)


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

    def batch(spec, samples, db):
        return lambda: spec.batch_db(samples, rows, db)

    fns = {"r": batch(real, x, out[0]), "c": batch(cplx, iq, out[1]), "b": batch(cplx2, iq, out[1])}
    rr, rc = timing.reps_for(fns["r"], args.seconds), timing.reps_for(fns["c"], args.seconds)
    timing.reps_for(fns["b"], args.seconds)
    same = float((out[0] - out[1]).abs().max())           # (dB rows of the two paths, everywhere: noise-floor bins included)
    reps = {"r": rr, "c": rc, "b": rc}
    got = timing.alternate({"c": fns["c"], "b": fns["b"]}, reps, args.windows, timing.MS)   # the same code against itself
    a, b = got["c"], got["b"]
    got = timing.alternate({"r": fns["r"], "c": fns["c"]}, reps, args.windows, timing.MS)   # real against IQ with zeros
    r, c = got["r"], got["c"]
    print(json.dumps({"fft_size": n, "rows": rows, "windows": args.windows, "reps_per_window": {"real": rr, "iq": rc},
                      "iq_ms_per_batch_a": summary(a), "iq_ms_per_batch_b": summary(b),
                      "spread_same_code": timing.spread(a, b),
                      "real_ms_per_batch": summary(r), "iq_zero_q_ms_per_batch": summary(c),
                      "real_over_iq": round(statistics.median(r) / statistics.median(c), 4),
                      "max_db_difference_real_vs_iq": round(same, 5)}), flush=True)
    for s in (real, cplx, cplx2):
        s.destroy()
    del x, iq, out, t, fns
    torch.cuda.empty_cache()
dev.close()
