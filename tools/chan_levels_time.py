"""Timing of wr_tuner_chan_levels -- every receiver's signal level out of the tuner's channel IQ, one pass over it --
against the only route there was before it, against one wr_tuner_chan_spectra, and against a plain copy of the same
bytes (development aid; bench.py is the contract).  profiles/chan_levels.txt was taken with it.

  python tools/chan_levels_time.py [--windows 8] [--seconds 0.2]

One process, one device.  BASELINE config 2's shape: 256 receivers off 100 Msps, one block of 4 000 000 frames, 10 000
channel-rate frames per receiver (20.48 MB of channel IQ).  Once with no squelch in use and once with one on every
receiver (the kernel then also counts the muted audio frames).  Figures, all between two device events over repeated
calls, the four ALTERNATING window by window:
  levels     one wr_tuner_chan_levels call.  The call is synchronous: two kernels, one copy of 3 KB to the host and the
             wait for it, so the figure is the whole call as a caller pays it, not the kernels alone (those: a
             rocprofv3 --kernel-trace --stats run of this tool);
  levels_b   the same call again: the spread below which a difference means nothing;
  spectra    one wr_tuner_chan_spectra at 512 points (asynchronous: the launch alone);
  copy       a device-to-device copy of the same 20.48 MB: the price of touching those bytes once;
and with a host clock:
  per_chan   256 x wr_chan_fetch(WR_STAGE_CHAN_IQ) plus the sum in numpy: what there was.
Prints one JSON line per case."""
import json
import statistics
import time

import timing

ap = timing.parser()
ap.add_argument("--per-chan-rounds", type=int, default=2)
args = timing.parse(ap)

import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402
from webradio_amd import capi, synth                      # noqa: E402
from webradio_amd.device import Spectrum                  # noqa: E402

C2 = synth.C2
NRX, NFRAMES = C2["channels"], C2["block_frames"]
K1 = NFRAMES // (C2["input_rate"] // C2["chan_rate"])
BYTES = K1 * NRX * 8

dev, ifs, block = timing.c2_case()
tuner, chans = timing.c2_tuner(dev, ifs)
spec = Spectrum(dev, 512)
db = torch.empty(NRX * 512, device="cuda")
copy = timing.copier(BYTES)


def levels():
    tuner.chan_levels()


def spectra():
    tuner.chan_spectra(spec, K1 - 512, db_dev=db)


for squelch in (False, True):
    for ch in chans:
        tuner.set_squelch(ch, -30.0, squelch)
    tuner.submit_device(block, NFRAMES)
    tuner.flush()
    torch.cuda.synchronize()
    mean, peak, muted, frames, audio_frames = tuner.chan_levels()
    assert frames == K1 and mean.size == NRX
    rl, rs, rc = (timing.reps_for(fn, args.seconds) for fn in (levels, spectra, copy))
    got = timing.alternate({"a": levels, "s": spectra, "b": levels, "c": copy}, {"a": rl, "s": rs, "b": rl, "c": rc}, args.windows)
    a, b, s, c = got["a"], got["b"], got["s"], got["c"]
    per, worst = [], 0.0
    for rnd in range(args.per_chan_rounds + 1):
        t0 = time.perf_counter()
        for ch in chans:
            iq = tuner.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * K1).reshape(-1, 2)
            m = float((iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]).sum(dtype=np.float64)) / K1
            if rnd == 0 and m > 0.0:                      # (warm-up round: also where the two routes are compared)
                worst = max(worst, abs(float(mean[tuner.slot(ch)]) - m) / m)
        if rnd:
            per.append((time.perf_counter() - t0) * 1e6)
    med = statistics.median(a + b)
    print(json.dumps({"squelch_on_every_receiver": squelch, "receivers": NRX, "k1": K1, "bytes": BYTES,
                      "muted_frames_min_max": [int(muted.min()), int(muted.max())], "audio_frames": audio_frames,
                      "windows": args.windows, "reps_per_window": {"levels": rl, "spectra": rs, "copy": rc},
                      "levels_us_per_call": timing.summary(a), "levels_b_us_per_call": timing.summary(b),
                      "spread_same_code": timing.spread(a, b),
                      "spectra_512_us_per_call": timing.summary(s), "copy_us": timing.summary(c),
                      "levels_GB_per_s_whole_call": round(BYTES / med / 1e3, 1),
                      "copy_GB_per_s_read_plus_write": round(2 * BYTES / statistics.median(c) / 1e3, 1),
                      "levels_over_copy": round(med / statistics.median(c), 3),
                      "per_chan_route_us_for_all": timing.summary(per),
                      "per_chan_route_over_levels": round(statistics.median(per) / med, 1),
                      "max_relative_difference_of_the_means": float("%.3g" % worst)}), flush=True)
spec.destroy()
tuner.destroy()
dev.close()
