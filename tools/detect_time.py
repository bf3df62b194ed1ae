"""Timing of wr_spectrum_rows_detect -- noise floors and occupied segments of spectrum rows -- against a plain copy of the same
rows and against wr_spectrum_rows_waterfall on the same rows, all in the same run (development aid; bench.py is the contract).
profiles/detect.txt is where its figures go.

  python tools/detect_time.py [--windows 8] [--seconds 0.2]

One process, one device.  Figures, all between two device events over repeated calls, ALTERNATING window by window.  Three
shapes of dB rows (averaged noise near -40 dB, a carrier every 4096 bins or two a row), the default rule:
  row64k   one 65536-point row, spans of 1024: the waterfall's mean row;
  audio    256 rows x 256: the audio spectra of all receivers;
  chan     256 rows x 1024: the channel spectra;
and, once, the top size:
  row1m    one 1048576-point row in spans of 1024, and the same row as ONE span (the select re-reads 4 MB four times, in one
           workgroup; the segments are one workgroup's 1024 tiles either way).
Per shape: detect (the call, floors in the spectrum's scratch, 64 records a row), detect_b (the same again: the spread below
which a difference means nothing), copy (device to device, the rows' bytes), waterfall (rows_waterfall to 256 columns, hold 1,
both outputs).  The two kernels' own times come from rocprofv3 --kernel-trace --stats on this tool.  Prints one JSON line."""
import json
import statistics

import timing

args = timing.parse(timing.parser())

import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402
from webradio_amd.device import DETECTION, Spectrum       # noqa: E402

MAX_DET = 64
dev = timing.open_device()
rng = np.random.default_rng(1)


def rows_of(nrows, n):
    p = rng.exponential(1.0, (16, nrows * n)).mean(axis=0) * 1e-4
    p[:: min(4096, n // 2)] *= 1e3
    return torch.from_numpy((10.0 * np.log10(p)).astype(np.float32)).cuda()


def shape(name, nrows, n, width, **rule_fields):
    spec = Spectrum(dev, n)
    rows = rows_of(nrows, n)
    rule = spec.detect_rule(**rule_fields)
    det = torch.empty(nrows * MAX_DET * DETECTION.itemsize, dtype=torch.uint8, device="cuda")
    count = torch.empty(nrows, dtype=torch.int32, device="cuda")
    wdb = torch.empty(nrows * width, device="cuda")
    wpal = torch.empty(nrows * width, dtype=torch.uint8, device="cuda")

    def detect():
        spec.rows_detect(rows, nrows, rule, MAX_DET, det, count)

    fns = {"detect": detect, "detect_b": detect, "copy": timing.copier(4 * nrows * n),
           "waterfall": lambda: spec.rows_waterfall(rows, nrows, width, 1, wdb, wpal)}
    got, reps = timing.measure(fns, args)
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in got.items()}
    both = 0.5 * (med["detect"] + med["detect_b"])
    out = {"rows": nrows, "n": n, "span": rule.span, "bytes": 4 * nrows * n, "kept_segments": int(count.sum().item()),
           "reps_per_window": reps, **{k + "_us": timing.summary(v) for k, v in got.items()},
           "spread_same_code": timing.spread(got["detect"], got["detect_b"]),
           "detect_over_copy": round(both / med["copy"], 3), "detect_over_waterfall": round(both / med["waterfall"], 3)}
    spec.destroy()
    return name, out


result = dict([shape("row64k", 1, 65536, 256), shape("audio", 256, 256, 256), shape("chan", 256, 1024, 256),
               shape("row1m", 1, 1 << 20, 256), shape("row1m_one_span", 1, 1 << 20, 256, span=1 << 20)])
print(json.dumps({"windows": args.windows, "max_det": MAX_DET, **result}), flush=True)
dev.close()
