"""wr_tuner_chan_levels' rule of summation, restated in numpy float32 (include/webradio_amd.h): e = i*i + q*q per
frame (two products and one sum, each rounded); frames added oldest first in runs of 16, the run sums in order in groups
of 16 runs, the group sums in order; the last run and the last group simply shorter; every partial starts from its
first term.  test_chan_levels_capi.py holds it to float64 without a GPU, test_gpu_chan_levels.py holds the kernels to it."""
import math

import numpy as np


def power(iq):
    z = np.asarray(iq, np.float32).reshape(-1, 2)
    return (z[:, 0] * z[:, 0]).astype(np.float32) + (z[:, 1] * z[:, 1]).astype(np.float32)


def _fold(v, n):
    """sums of consecutive runs of n values, each added in order from its first term; the last run may be shorter"""
    full = v.size // n
    out = np.empty((v.size + n - 1) // n, np.float32)
    if full:
        a = v[:full * n].reshape(full, n)
        acc = a[:, 0].copy()
        for i in range(1, n):
            acc = acc + a[:, i]                      # float32 + float32, rounded once
        out[:full] = acc
    if full < out.size:
        t = v[full * n]
        for x in v[full * n + 1:]:
            t = np.float32(t + x)
        out[full] = t
    return out


def levels(iq):
    """(mean, peak) of a block of IQ frames, as float32 scalars"""
    e = power(iq)
    assert e.dtype == np.float32 and e.size
    total = _fold(_fold(_fold(e, 16), 16), 1 << 62)[0]
    return np.float32(total / np.float32(e.size)), np.float32(e.max())


def mean_bound(k1):
    """relative distance of levels()[0] from the float64 mean of the same frames: at most 15 + 15 + ceil(k1/256) - 1
    additions in the chain a term passes through, two roundings inside e (a product, then the sum of the two) and one
    division, all on non-negative terms, half an ulp (2^-24) each -- with slack for the second-order terms"""
    return (34 + math.ceil(k1 / 256)) * 2.0 ** -24


def mean_f64(iq):
    z = np.asarray(iq, np.float32).reshape(-1, 2).astype(np.float64)
    return float((z[:, 0] ** 2 + z[:, 1] ** 2).mean())


def bits(a):
    """the uint32 behind float32 values: an int for a scalar, an array for an array"""
    u = np.asarray(a, np.float32).view(np.uint32)
    return int(u) if u.ndim == 0 else u
