"""What the *_time.py tools share (development aids; bench.py is the contract): the command line, a figure between two device
events, windows that alternate between the things compared, and BASELINE config 2's tuner.  Importing it does nothing; torch
and the package are imported where they are used, after parse() has put --root on the path.

  ap = timing.parser(); ap.add_argument(...); args = timing.parse(ap)
  got, reps = timing.measure({"this": f, "that": g}, args)          # per-window figures and calls per window, by name
"""
import argparse
import os
import statistics
import sys

US, MS = 1e3, 1.0                                         # a figure's unit: how many of it make a millisecond


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap


def parse(ap):
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    return args


def per_call(fn, reps, unit=US):
    """`reps` calls between two device events: the time per call"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * unit / reps


def reps_for(fn, seconds):
    """how many calls fill a window of `seconds`: at least 8"""
    import torch
    for _ in range(3):                                    # warm-up: code objects, uploads, LDS attributes, scratch buffers
        fn()
    torch.cuda.synchronize()
    return max(8, int(seconds * 1e3 / per_call(fn, 20, MS)) + 1)


def summary(values, digits=2):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits),
            "max": round(max(values), digits)}


def spread(a, b):
    """the same code against itself, window by window: the difference below which one means nothing"""
    return round(max(abs(u / v - 1.0) for u, v in zip(a, b)), 4)


def alternate(fns, reps, windows, unit=US):
    """{name: [figure per window]}: every window runs each of `fns` in turn, reps[name] calls of it"""
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(per_call(fn, reps[k], unit))
    return got


def measure(fns, args, unit=US):
    """alternate() with every name's calls per window found by reps_for; (figures, reps)"""
    reps = {k: reps_for(fn, args.seconds) for k, fn in fns.items()}
    return alternate(fns, reps, args.windows, unit), reps


def copier(nbytes):
    """a device-to-device copy of `nbytes`: the price of touching those bytes once"""
    import torch
    src = torch.randn(nbytes // 4, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


# ---- BASELINE config 2: 256 receivers off 100 Msps, blocks of 4 000 000 frames -------------------------------------------------

def open_device():
    import torch
    from webradio_amd.device import Device
    return Device(0, torch.cuda.current_stream().cuda_stream)


def c2_case():
    """(device, the 256 IFs, one block in device memory: a carrier on every eighth receiver over noise at -50 dBFS)"""
    from webradio_amd import synth
    ifs = synth.c2_ifs()
    return open_device(), ifs, synth.fm_stream_torch(synth.C2["block_frames"], synth.C2["input_rate"], ifs[::8], "cuda",
                                                     noise_dbfs=-50.0)


def c2_tuner(dev, ifs, agc=False):
    """(tuner, channels): config 2's NFM receivers, streaming off; with `agc`, the default AGC on every one"""
    from webradio_amd import capi, synth
    from webradio_amd.device import Tuner
    C2 = synth.C2
    t = Tuner(dev, C2["input_rate"], C2["channels"], C2["block_frames"])
    chans = [t.add_receiver(f, C2["chan_passband"], C2["chan_rate"], capi.WR_FM, C2["audio_passband"], C2["audio_rate"])
             for f in ifs]
    if agc:
        for ch in chans:
            t.set_agc(ch)
    return t, chans


def row_bank_figures(args, dev, ifs, block, push, rows_n, nbytes, beside=None):
    """The figures tones_time.py, dcs_time.py and resamp_time.py share, as the fields of their JSON line behind the shape's
    own: rows_256 / rows_64 (`rows_n(n)`: the plain-rows call on n rows), submit_push (`push(tuner)` behind a submit),
    submit_flush and submit_plain(_b) on twin tuners, copy (`nbytes`), and what is derived from their medians.
    `beside`: {name: call} timed in the same windows, to set the figures beside."""
    import torch
    nframes = block.numel() // 2
    pushed, flushed, plain = (c2_tuner(dev, ifs)[0] for _ in range(3))

    def submit_push():
        pushed.submit_device(block, nframes)
        push(pushed)

    def submit_flush():
        flushed.submit_device(block, nframes)
        flushed.flush()

    def submit_plain():
        plain.submit_device(block, nframes)

    fns = {"rows_256": rows_n(256), "rows_64": rows_n(64), "submit_push": submit_push, "submit_flush": submit_flush,
           "submit_plain": submit_plain, "submit_plain_b": submit_plain, "copy": copier(nbytes), **(beside or {})}
    got, reps = measure(fns, args)
    for t in (pushed, flushed, plain):
        t.flush()
    torch.cuda.synchronize()
    for t in (pushed, flushed, plain):
        t.destroy()
    med = {k: statistics.median(v) for k, v in got.items()}
    plain_us = 0.5 * (med["submit_plain"] + med["submit_plain_b"])
    return {"bytes": nbytes, "windows": args.windows, "reps_per_window": reps, **{k + "_us": summary(v) for k, v in got.items()},
            "spread_same_code": spread(got["submit_plain"], got["submit_plain_b"]),
            "push_in_a_submit_us": round(med["submit_push"] - plain_us, 2),
            "push_over_a_flush_us": round(med["submit_push"] - med["submit_flush"], 2),
            "rows_64_over_rows_256": round(med["rows_64"] / med["rows_256"], 3),
            "rows_256_over_copy": round(med["rows_256"] / med["copy"], 3)}
