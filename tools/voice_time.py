"""Timing of the voice bank -- wr_voice_push_rows on a plain block of rows, and wr_tuner_voice_push behind a submit -- against
the same submit without it, against a plain copy of the same bytes and against the resampler on the same rows (development
aid; bench.py is the contract).  profiles/voice.txt is where its figures go.

  python tools/voice_time.py [--windows 8] [--seconds 0.2]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, blocks of 4 000 000 frames, 2 000 audio
frames per receiver and block (2.05 MB of audio) at 50 kHz, streaming off in all tuners.  Figures, all between two device
events over repeated calls, ALTERNATING window by window; the taps are wr_voice_design's 300 .. 3000 Hz band-pass (with
750 us of de-emphasis from 1024 taps on), every row on filter 0:
  rows_256, rows_64     one wr_voice_push_rows call of 1024 taps on 256 x 2 000 and on 64 x 2 000 frames (timing.py);
  rows_256_t256, rows_256_t2048    the same on 256 x 2 000 with 256 and with 2048 taps;
  rows_256x640_t512     256 x 640 frames with 512 taps: the bank behind the resampler, at 16 kHz;
  resamp_256, resamp_64 wr_resamp_push_rows (24 / 25, 32 taps per phase) on the same rows;
  copy                  a device-to-device copy of the same 2.05 MB: the price of touching those bytes once;
  submit_push           one wr_tuner_submit of a device block followed by wr_tuner_voice_push with 1024 taps;
  submit_push_t256, submit_push_t2048, submit_push_64   the same with 256 and 2048 taps, and on a tuner of 64 receivers
                        (1024 taps) beside submit_plain_64, that tuner's submit alone;
  submit_flush, submit_plain(_b)   as in resamp_time.py.
`ceiling_us` is arithmetic: 2 rows frames T unfused, unpacked lane operations against a quarter of the vector peak
(157.3 TF / 4).  Prints one JSON line."""
import json
import statistics

import timing

args = timing.parse(timing.parser())

import torch                                               # noqa: E402
from webradio_amd import capi, synth                       # noqa: E402
from webradio_amd.device import Resampler, VoiceBank, voice_design   # noqa: E402

C2 = synth.C2
NRX, NFRAMES, RATE = C2["channels"], C2["block_frames"], C2["audio_rate"]
K2 = NFRAMES // (C2["input_rate"] // RATE)
PEAK_OVER_FOUR = 157.3e12 / 4.0

dev, ifs, block = timing.c2_case()
rows = 0.05 * torch.randn(NRX * K2, device="cuda")
out = torch.empty(NRX * K2, device="cuda")
slots = capi.C.c_uint()


def bank_of(T, rate=RATE):
    return VoiceBank(dev, NRX, voice_design(rate, T, 300, 3000, 750 if T >= 1024 else 0))


banks = {T: bank_of(T) for T in (256, 1024, 2048)}                 # ... of the tuner pushes
row_banks = {T: bank_of(T) for T in (256, 1024, 2048)}             # ... of the plain rows
row_banks[512] = bank_of(512, 16_000)
rs = Resampler(dev, NRX, RATE, 48_000, 32)
n_out = rs.out_frames(K2) + 1
rs_out = torch.empty(NRX * n_out, device="cuda")


def rows_call(T, nrows, nframes=K2):
    return lambda: row_banks[T].push_rows(rows.data_ptr(), K2, nrows, nframes, out.data_ptr(), K2)


def tuner_push(T):
    return lambda tuner: capi.check(dev.lib.wr_tuner_voice_push(tuner.h, banks[T].h, capi.ptr(out), K2, capi.C.byref(slots)))


def submit_then(tuner, push=None):
    def call():
        tuner.submit_device(block, NFRAMES)
        if push:
            push(tuner)
    return call


def tuner_of(n):
    """config 2's tuner with its first n receivers"""
    from webradio_amd.device import Tuner
    t = Tuner(dev, C2["input_rate"], n, NFRAMES)
    for f in ifs[:n]:
        t.add_receiver(f, C2["chan_passband"], C2["chan_rate"], capi.WR_FM, C2["audio_passband"], RATE)
    return t


extra = {"t256": timing.c2_tuner(dev, ifs)[0], "t2048": timing.c2_tuner(dev, ifs)[0], "64": tuner_of(64), "plain_64": tuner_of(64)}
bank_64 = VoiceBank(dev, 64, voice_design(RATE, 1024, 300, 3000, 750))
beside = {"rows_256_t256": rows_call(256, NRX), "rows_256_t2048": rows_call(2048, NRX), "rows_256x640_t512": rows_call(512, NRX, 640),
          "resamp_256": lambda: rs.push_rows(rows.data_ptr(), K2, NRX, K2, rs_out.data_ptr(), n_out),
          "resamp_64": lambda: rs.push_rows(rows.data_ptr(), K2, 64, K2, rs_out.data_ptr(), n_out),
          "submit_push_t256": submit_then(extra["t256"], tuner_push(256)),
          "submit_push_t2048": submit_then(extra["t2048"], tuner_push(2048)),
          "submit_push_64": submit_then(extra["64"], lambda tuner: capi.check(dev.lib.wr_tuner_voice_push(
              tuner.h, bank_64.h, capi.ptr(out), K2, capi.C.byref(slots)))),
          "submit_plain_64": submit_then(extra["plain_64"])}
figures = timing.row_bank_figures(args, dev, ifs, block, tuner_push(1024), lambda n: rows_call(1024, n), K2 * NRX * 4, beside)
for t in extra.values():
    t.flush()
torch.cuda.synchronize()
assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
for t in extra.values():
    t.destroy()
med = {k[:-3]: v["median"] for k, v in figures.items() if k.endswith("_us") and isinstance(v, dict)}
plain_us = 0.5 * (med["submit_plain"] + med["submit_plain_b"])
shapes = {"rows_256_t256": (NRX, K2, 256), "rows_256": (NRX, K2, 1024), "rows_256_t2048": (NRX, K2, 2048), "rows_64": (64, K2, 1024),
          "rows_256x640_t512": (NRX, 640, 512)}
ceiling = {k: round(2.0 * r * n * T / PEAK_OVER_FOUR * 1e6, 2) for k, (r, n, T) in shapes.items()}
print(json.dumps({"receivers": NRX, "k2": K2, **figures, "ceiling_us": ceiling,
                  "over_ceiling": {k: round(med[k] / ceiling[k], 2) for k in shapes},
                  "push_in_a_submit_t256_us": round(med["submit_push_t256"] - plain_us, 2),
                  "push_in_a_submit_t2048_us": round(med["submit_push_t2048"] - plain_us, 2),
                  "push_in_a_submit_64_us": round(med["submit_push_64"] - med["submit_plain_64"], 2),
                  "rows_256_over_resamp_256": round(med["rows_256"] / med["resamp_256"], 2),
                  "rows_64_over_resamp_64": round(med["rows_64"] / med["resamp_64"], 2)}), flush=True)
for b in list(banks.values()) + list(row_banks.values()) + [bank_64]:
    b.destroy()
rs.destroy()
dev.close()
