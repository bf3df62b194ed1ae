"""Timing of wr_spectrum_batch_avg -- mean and peak-hold rows over all frames of a block -- against wr_spectrum_batch_db on
the same frames and against a plain copy of the same input bytes (development aid; bench.py is the contract).
profiles/spectrum_avg.txt is where its figures go.

  python tools/spectrum_avg_time.py [--windows 8] [--seconds 0.2]

One process, one device.  Figures, all between two device events over repeated calls, ALTERNATING window by window:
  avg_c3        one wr_spectrum_batch_avg call on BASELINE config 3's shape: 65536 points, hop 32768, all whole frames of
                one block of 4 000 000 frames (121), mean and peak rows in dB;
  db_c3         wr_spectrum_batch_db on the same frames (121 dB rows): the yardstick;
  db_c3_b       the same again: the spread below which a difference means nothing;
  copy_c3       a device-to-device copy of the block's 32 MB;
  avg_audio     the averaged audio spectra of 256 rows x 2 000 frames (real, 256 points, hop 128: 14 frames a row), one call;
  db_rows_audio wr_spectrum_batch_db_rows on the same rows (the first 256 frames of each: one transform a row);
  copy_audio    a device-to-device copy of the rows' 2.05 MB.
Prints one JSON line."""
import json
import statistics

import timing

args = timing.parse(timing.parser())

import torch                                              # noqa: E402
from webradio_amd.device import Spectrum                  # noqa: E402

N3, HOP3, BLOCK = 65536, 32768, 4_000_000
F3 = (BLOCK - N3) // HOP3 + 1
NA, HOPA, ROWS, K2 = 256, 128, 256, 2000
FA = (K2 - NA) // HOPA + 1

dev = timing.open_device()
block = torch.randn(2 * BLOCK, device="cuda") * 0.1
audio = torch.randn(ROWS * K2, device="cuda") * 0.1
c3, aud = Spectrum(dev, N3, HOP3), Spectrum(dev, NA, HOPA, real=True)
mean3, peak3 = torch.empty(N3, device="cuda"), torch.empty(N3, device="cuda")
rows3 = torch.empty(F3 * N3, device="cuda")
mean_a, peak_a, rows_a = (torch.empty(ROWS * NA, device="cuda") for _ in range(3))


def db_c3():
    c3.batch_db(block, F3, rows3)


fns = {"avg_c3": lambda: c3.batch_avg(block, F3, mean3, peak3),
       "db_c3": db_c3, "db_c3_b": db_c3, "copy_c3": timing.copier(8 * BLOCK),
       "avg_audio": lambda: aud.batch_avg(audio, FA, mean_a, peak_a, ROWS, K2),
       "db_rows_audio": lambda: aud.batch_db_rows(audio, K2, ROWS, rows_a),
       "copy_audio": timing.copier(4 * ROWS * K2)}
got, reps = timing.measure(fns, args)
torch.cuda.synchronize()
med = {k: statistics.median(v) for k, v in got.items()}
db3 = 0.5 * (med["db_c3"] + med["db_c3_b"])
print(json.dumps({"c3": {"n": N3, "hop": HOP3, "frames": F3, "bytes": 8 * BLOCK},
                  "audio": {"n": NA, "hop": HOPA, "rows": ROWS, "frames_per_row": FA, "bytes": 4 * ROWS * K2},
                  "windows": args.windows, "reps_per_window": reps,
                  **{k + "_us": timing.summary(v) for k, v in got.items()},
                  "spread_same_code": timing.spread(got["db_c3"], got["db_c3_b"]),
                  "avg_c3_over_db_c3": round(med["avg_c3"] / db3, 3),
                  "avg_c3_minus_db_c3_us": round(med["avg_c3"] - db3, 2),
                  "avg_c3_over_copy": round(med["avg_c3"] / med["copy_c3"], 3),
                  "avg_audio_over_db_rows_audio": round(med["avg_audio"] / med["db_rows_audio"], 3)}), flush=True)
c3.destroy()
aud.destroy()
dev.close()
