"""The AGC rule of include/webradio_amd.h (wr_agc_rows) restated in numpy, in two forms: `envelope_loop`, the rule as a
plain Python loop, and `envelope`, its closed form as a prefix maximum on int64 -- the envelope is integer arithmetic, so
the two, and the GPU's, have the same bits -- plus `apply`, the float32 division and products, and `design`,
wr_agc_design's arithmetic."""
import math

import numpy as np

OFF = 0xFFFFFFFF                   # step: a row without AGC
FLT_MAX_BITS = 0x7F7FFFFF


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def level(v):
    """L[m] = min(bits(v[m]) & 0x7fffffff, 0x7f7fffff), as int64"""
    return np.minimum(bits(v) & np.uint32(0x7FFFFFFF), np.uint32(FLT_MAX_BITS)).astype(np.int64)


def envelope_loop(v, floor_bits, step, state):
    """E[m] = max(L[m], E[m-1] - step, floor) one frame after the other; E[-1] = state.  Returns (E as uint32, last E)."""
    e = int(state)
    out = np.empty(len(v), np.uint32)
    for m, l in enumerate(level(v)):
        e = max(int(l), e - int(step), int(floor_bits))
        out[m] = e
    return out, e


def envelope(v, floor_bits, step, state):
    """the same by the closed form: E[m] = max(max_{j<=m}(L[j] + j step) - m step, state - (m+1) step, floor)"""
    n = len(v)
    if not n:
        return np.empty(0, np.uint32), int(state)
    m = np.arange(n, dtype=np.int64)
    u = np.maximum.accumulate(level(v) + m * int(step)) - m * int(step)
    e = np.maximum(np.maximum(u, int(state) - (m + 1) * int(step)), int(floor_bits))
    return e.astype(np.uint32), int(e[-1])


def apply(v, target, floor_bits, step, state, af_gain=1.0, scale=1.0):
    """out[m] = v[m] * (target / env[m]), then * af_gain if it is not 1, then * scale if it is not 1, every operation in
    float32.  Returns (out, last E)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    e, last = envelope(v, floor_bits, step, state)
    with np.errstate(all="ignore"):
        g = np.float32(target) / e.view(np.float32)
        out = v * g
        if np.float32(af_gain) != np.float32(1.0):
            out = out * np.float32(af_gain)
        if np.float32(scale) != np.float32(1.0):
            out = out * np.float32(scale)
    assert out.dtype == np.float32
    return out, last


def design(target_dbfs, decay_db_per_s, max_gain_db, audio_rate):
    """(target float32, floor_bits, step) as wr_agc_design gives them: the dB values as float32, the rest in double"""
    t, d, g = (float(np.float32(x)) for x in (target_dbfs, decay_db_per_s, max_gain_db))
    lvl = math.pow(10.0, t / 20.0)
    floor = np.float32(lvl / math.pow(10.0, g / 20.0))
    per_frame = d / (20.0 * math.log10(2.0)) * 8388608.0 / float(audio_rate)
    step = min(int(math.floor(per_frame + 0.5)), 1 << 31)          # llround: halves away from zero (the value is >= 0)
    return np.float32(lvl), int(bits(floor)[0]), step
