"""Timing of wr_tuner_chan_spectra -- every receiver's channel spectrum out of the tuner's channel IQ, read as columns --
against the same transforms on rows, and against the only route there was before it (development aid; bench.py is the
contract).  profiles/chan_spectra.txt was taken with it.

  python tools/chan_spectra_time.py [--windows 8] [--seconds 0.2] [--sizes 512,2048,8192]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, one block of 4 000 000 frames, 10 000
channel-rate frames per receiver.  Per size three figures:
  columns    one wr_tuner_chan_spectra call (256 dB rows), between two device events over repeated calls;
  rows       wr_spectrum_batch_db_rows on 256 CONTIGUOUS IQ rows of the same size, the same way: the two ALTERNATE window
             by window, so the ratio is the cost of the column layout alone.  The first pair of figures per size is the
             row path against itself: the spread below which a difference means nothing;
  per_chan   256 x (wr_chan_fetch(WR_STAGE_CHAN_IQ) + wr_spectrum_push from the host + wr_spectrum_get_db), a host clock
             around calls that each end in a synchronise.
Prints one JSON line per size."""
import json
import statistics
import time

import timing

ap = timing.parser()
ap.add_argument("--sizes", default="512,2048,8192")
ap.add_argument("--per-chan-rounds", type=int, default=3)
args = timing.parse(ap)

import torch                                              # noqa: E402
from webradio_amd import capi, synth                      # noqa: E402
from webradio_amd.device import Spectrum                  # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K1 = NFRAMES // (C2["input_rate"] // C2["chan_rate"])

dev, ifs, block = timing.c2_case()
tuner, chans = timing.c2_tuner(dev, ifs)
tuner.submit_device(block, NFRAMES)
tuner.flush()
torch.cuda.synchronize()


def summary(ms):
    return timing.summary(ms, 5)


for n in (int(s) for s in args.sizes.split(",")):
    first = K1 - n
    spec, spec2, one = Spectrum(dev, n), Spectrum(dev, n), Spectrum(dev, n)
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    rows_iq = torch.randn(2 * NRX * n, device="cuda", generator=g) * 0.1     # 256 contiguous IQ rows of n frames
    out = [torch.empty(NRX * n, device="cuda") for _ in range(2)]

    def columns():
        tuner.chan_spectra(spec, first, db_dev=out[0])

    def rows():
        spec.batch_db_rows(rows_iq, n, NRX, out[1])

    def rows2():
        spec2.batch_db_rows(rows_iq, n, NRX, out[1])

    rc, rr = timing.reps_for(columns, args.seconds), timing.reps_for(rows, args.seconds)
    timing.reps_for(rows2, args.seconds)
    reps = {"a": rr, "b": rr, "c": rc, "r": rr}
    same = timing.alternate({"a": rows, "b": rows2}, reps, args.windows, timing.MS)          # the same code against itself
    got = timing.alternate({"c": columns, "r": rows}, reps, args.windows, timing.MS)          # columns against rows
    a, b, c, r = same["a"], same["b"], got["c"], got["r"]

    # the route there was: per receiver one gather kernel, one copy to the host, one synchronise -- and the frame back up
    want = tuner.chan_spectra(spec, first)
    per, worst = [], 0.0
    for rnd in range(args.per_chan_rounds + 1):
        t0 = time.perf_counter()
        for ch in chans:
            iq = tuner.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * K1)
            one.push_host(iq[2 * first: 2 * (first + n)])
            db = one.get_db()
            if rnd == 0:                                  # (warm-up round: also where the two routes are compared)
                w = want[tuner.slot(ch)]
                strong = w >= w.max() - 60.0
                worst = max(worst, float(abs(db[strong] - w[strong]).max()))
        if rnd:
            per.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"fft_size": n, "receivers": NRX, "k1": K1, "first_frame": first, "windows": args.windows,
                      "reps_per_window": {"columns": rc, "rows": rr},
                      "rows_ms_a": summary(a), "rows_ms_b": summary(b), "spread_same_code": timing.spread(a, b),
                      "columns_ms_per_call": summary(c), "rows_ms_per_call": summary(r),
                      "columns_over_rows": round(statistics.median(c) / statistics.median(r), 4),
                      "per_chan_route_ms_for_all": summary(per),
                      "per_chan_route_over_columns": round(statistics.median(per) / statistics.median(c), 1),
                      "max_db_difference_on_strong_bins": round(worst, 6)}), flush=True)
    for s in (spec, spec2, one):
        s.destroy()
    del rows_iq, out
    torch.cuda.empty_cache()
tuner.destroy()
dev.close()
