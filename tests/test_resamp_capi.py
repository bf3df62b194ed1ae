"""The resampler without a GPU: the nine functions are declared and bound with the same argument counts, the header carries
the rule, NULL handles are refused by name, wr_resamp_ratio and wr_resamp_design give numpy's numbers and filters that meet
the stated conditions, and the restatement the GPU tests compare bits with (tests/resamp_np.py) is held here first to the
rule written as plain loops (bit for bit, for any cut into pushes) and to an ideal sine delayed by the group delay."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import capicases
import resamp_np
from webradio_amd import capi

NAMES = [("wr_resamp_ratio", 4), ("wr_resamp_design", 6), ("wr_resamp_create", 7), ("wr_resamp_destroy", 1),
         ("wr_resamp_reset", 2), ("wr_resamp_out_frames", 3), ("wr_resamp_push_rows", 8), ("wr_resamp_info", 6),
         ("wr_tuner_resamp_push", 6)]
DESIGNS = [(50_000, 48_000, 16), (50_000, 48_000, 32), (50_000, 48_000, 64), (32_000, 48_000, 32), (50_000, 44_100, 32),
           (32_000, 44_100, 32), (250_000, 48_000, 64), (8_000, 48_000, 32), (48_000, 8_000, 64), (1_000, 750, 32)]
SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, -0.0, 1e-40, 65536.0]


@pytest.mark.parametrize("name, nargs", NAMES)
def test_declared_and_bound_with_the_same_arguments(name, nargs):
    capicases.declared_and_bound(name, nargs)


def test_header_says_the_rule():
    text = capicases.header()
    assert re.search(r"#define\s+WR_ABI_VERSION\s+6\b", text)
    assert re.search(r"Added to 6 later: wr_resamp_ratio, wr_resamp_design, wr_resamp_create, wr_resamp_destroy,\s+"
                     r"wr_resamp_reset, wr_resamp_out_frames, wr_resamp_push_rows,\s+wr_resamp_info, wr_tuner_resamp_push\.", text)
    for word in ("x'   = 0.0f if (bits(x) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else min(max(x, -65536.0f), 65536.0f)",
                 "t = m * M, n0 = t / L (floor), ph = t mod L", "acc  = +0.0f",
                 "for k = 0 ... P-1 in this order:  acc = acc + c[ph][k] * x'[n0 - k]", "y[m] = acc",
                 "ceil(N1 * L / M) - ceil(N0 * L / M)", "Only N mod M is needed", "1 <= L <= 1024", "1 <= M <= 8 L and L <= 8 M",
                 "L * P <= 16384", "c[ph][k] = h[k * L + ph]", "an int16 output", "host-side C++ class", "per-row ratios",
                 "clock-drift tracking", "inside the streaming launch", "time sharding"):
        assert word in text, word


def test_the_package_exports_the_names():
    import webradio_amd
    from webradio_amd import device
    assert webradio_amd.Resampler is device.Resampler and webradio_amd.resamp_design is device.resamp_design
    assert hasattr(device.Tuner, "resamp_push")


def test_null_handles_are_refused():
    lib = capi.load()
    a = np.zeros(16, np.float32)
    h, u, n = C.c_void_p(), C.c_uint(), C.c_size_t()
    for call, name in ((lambda: lib.wr_resamp_create(C.byref(h), None, 1, 1, 1, 4, capi.ptr(a)), b"wr_resamp_create"),
                       (lambda: lib.wr_resamp_create(None, None, 1, 1, 1, 4, capi.ptr(a)), b"wr_resamp_create"),
                       (lambda: lib.wr_resamp_reset(None, -1), b"wr_resamp_reset"),
                       (lambda: lib.wr_resamp_out_frames(None, 4, C.byref(n)), b"wr_resamp_out_frames"),
                       (lambda: lib.wr_resamp_push_rows(None, capi.ptr(a), 4, 1, 4, capi.ptr(a), 4, C.byref(n)),
                        b"wr_resamp_push_rows"),
                       (lambda: lib.wr_resamp_info(None, None, None, None, None, None), b"wr_resamp_info"),
                       (lambda: lib.wr_tuner_resamp_push(None, None, None, 0, None, None), b"wr_tuner_resamp_push"),
                       (lambda: lib.wr_resamp_ratio(3, 2, None, C.byref(u)), b"wr_resamp_ratio"),
                       (lambda: lib.wr_resamp_design(3, 2, 32, None, None, None), b"wr_resamp_design")):
        assert call() == capi.WR_ERR_ARG, name
        assert name in lib.wr_last_error(), (name, lib.wr_last_error())
    assert lib.wr_resamp_destroy(None) == capi.WR_OK


# ---- the design helper ----------------------------------------------------------------------------------------------------------

def _design(in_rate, out_rate, P, rows=1024):
    taps = np.full((rows, max(P, 1)), np.float32(np.nan), np.float32)
    L, M = C.c_uint(0xDEAD), C.c_uint(0xDEAD)
    rc = capi.load().wr_resamp_design(in_rate, out_rate, P, capi.ptr(taps), C.byref(L), C.byref(M))
    return rc, taps, L.value, M.value


@pytest.mark.parametrize("in_rate, out_rate, P", DESIGNS)
def test_design_equals_numpy(in_rate, out_rate, P):
    want, L, M = resamp_np.design(in_rate, out_rate, P)
    l, m = C.c_uint(), C.c_uint()
    assert capi.load().wr_resamp_ratio(in_rate, out_rate, C.byref(l), C.byref(m)) == capi.WR_OK
    assert (l.value, m.value) == (L, M) and math.gcd(L, M) == 1 and in_rate * L == out_rate * M
    rc, taps, L2, M2 = _design(in_rate, out_rate, P)
    assert rc == capi.WR_OK and (L2, M2) == (L, M)
    got = taps.reshape(-1)[: L * P].reshape(L, P)
    assert np.isnan(taps.reshape(-1)[L * P:]).all()                       # nothing written behind [L][P]
    # two evaluations of the same double formula, each rounded to float32 once
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print("%d -> %d, P %d: L / M %d / %d, max |c| %.4f, max difference %.3g" % (in_rate, out_rate, P, L, M, np.abs(want).max(), err))
    assert err <= 2.0 ** -23 * np.abs(want).max()


@pytest.mark.parametrize("in_rate, out_rate, P", DESIGNS)
def test_design_quality(in_rate, out_rate, P):
    """from the C helper's float taps, in float64: stopband <= -65 dB from min / 2, passband within -60 dB of 1 up to
    min / 2 - D (D = 5 in_rate / P), every phase's sum within 1e-4 of 1.  (Found with numpy's own design: -68.9 dB,
    -64.5 dB, 2.5e-5, max |c| < 0.9.)"""
    rc, taps, L, M = _design(in_rate, out_rate, P)
    assert rc == capi.WR_OK
    c = taps.reshape(-1)[: L * P].reshape(L, P).astype(np.float64)
    h = c.T.reshape(-1)                                                   # h[k L + ph]
    nfft = 1 << int(np.ceil(np.log2(64 * h.size)))
    mag = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(mag.size) * (L * in_rate / nfft)                        # Hz at the rate L * in_rate
    lo = min(in_rate, out_rate)
    width = 5.0 * in_rate / P
    stop = 20 * np.log10(mag[f >= lo / 2.0].max())
    ripple = 20 * np.log10(np.abs(mag[f <= lo / 2.0 - width] - 1.0).max())
    sums = np.abs(c.sum(axis=1) - 1.0).max()
    print("%d -> %d, P %d: stopband %.1f dB, passband deviation %.1f dB, phase sums within %.3g, max |c| %.3f" % (
        in_rate, out_rate, P, stop, ripple, sums, np.abs(c).max()))
    assert stop <= -65.0
    assert ripple <= -60.0
    assert sums <= 1e-4
    assert np.abs(c).max() < 16.0


@pytest.mark.parametrize("in_rate, out_rate, P", [(50_000, 48_000, 0), (50_000, 48_000, 2), (50_000, 48_000, 68),
                                                  (50_000, 48_000, 30),
                                                  (48_000, 1_000, 32),         # M > 8 L
                                                  (1_000, 48_000, 32),         # L > 8 M
                                                  (250_000, 48_000, 32),       # no passband: 48 000 <= 10 * 250 000 / 32
                                                  (44_100, 48_001, 32),        # L > 1024
                                                  (32_000, 44_100, 64),        # L * P = 28 224
                                                  (0, 48_000, 32), (48_000, 0, 32)])
def test_design_refuses(in_rate, out_rate, P):
    rc, taps, _, _ = _design(in_rate, out_rate, P, rows=16)
    assert rc == capi.WR_ERR_ARG
    assert b"wr_resamp_design" in capi.load().wr_last_error()
    assert np.isnan(taps).all()                                           # ... and nothing was written


def test_ratio_refuses_a_rate_of_zero():
    l, m = C.c_uint(), C.c_uint()
    assert capi.load().wr_resamp_ratio(0, 48_000, C.byref(l), C.byref(m)) == capi.WR_ERR_ARG
    assert capi.load().wr_resamp_ratio(48_000, 0, C.byref(l), C.byref(m)) == capi.WR_ERR_ARG


# ---- the restatement against the rule as plain loops ---------------------------------------------------------------------------

@pytest.mark.parametrize("in_rate, out_rate", [(32_000, 48_000), (50_000, 48_000), (1_000, 750), (50_000, 44_100)],
                         ids=["3/2", "24/25", "3/4", "441/500"])
def test_the_restatement_is_the_loop(in_rate, out_rate):
    P = 32
    taps, L, M = resamp_np.design(in_rate, out_rate, P)
    n = 400
    v = capicases.audio(n, L, SPECIAL, 7)
    bank, loop = resamp_np.Bank(1, L, M, taps), resamp_np.LoopBank(L, M, taps)
    pos, zero_seen = 0, False

    def push(length):
        nonlocal pos, zero_seen
        want_n = bank.out_frames(length)
        y = bank.push(v[None, pos: pos + length])
        z = loop.push(v[pos: pos + length])
        pos += length
        assert y.shape == (1, want_n) and capicases.same_bits(y[0], z), (L, M, pos, length)
        zero_seen = zero_seen or (want_n == 0)

    for length in (1, P - 2, P - 1):
        push(length)
    if L < M:                                                             # a push of one frame that yields no output
        while bank.out_frames(1):
            push(1)
        push(1)
        assert zero_seen
    push(0)                                                               # ... and, for every ratio, a push of nothing
    push(n - pos)
    assert bank.frames_in == n and bank.frames_out == loop.m == resamp_np.ceil_div(n * L, M)


def test_the_restatement_with_rough_taps_and_rows():
    """random taps up to +-16 with -0.0 and subnormals among them, three rows, a reset of one row in mid-stream and a push
    that leaves a row out: each row against its own loop"""
    L, M, P = 5, 7, 8
    rng = np.random.default_rng(9)
    taps = rng.uniform(-16, 16, (L, P)).astype(np.float32)
    taps[0, 0], taps[1, 3], taps[4, 7], taps[2, 2] = -0.0, 1e-40, -1e-42, 16.0
    v = np.stack([capicases.audio(120, 20 + r, SPECIAL, 7) for r in range(3)])
    bank = resamp_np.Bank(3, L, M, taps)
    loops = [resamp_np.LoopBank(L, M, taps) for _ in range(3)]
    y = bank.push(v[:, :50])
    for r in range(3):
        assert capicases.same_bits(y[r], loops[r].push(v[r, :50]))
    bank.reset(1)
    loops[1].reset_row()
    y = bank.push(v[:2, 50:53])                                           # row 2 is left out: it saw nothing
    loops[2].reset_row()
    loops[2].push(np.zeros(3, np.float32))
    for r in range(2):
        assert capicases.same_bits(y[r], loops[r].push(v[r, 50:53]))
    y = bank.push(v[:, 53:])
    for r in range(3):
        assert capicases.same_bits(y[r], loops[r].push(v[r, 53:])), r
    assert np.abs(y).max() <= 2.0 ** 26


def test_cleaning():
    got = resamp_np.clean(np.array(SPECIAL, np.float32))
    assert list(got[:5]) == [0.0, 0.0, 0.0, 65536.0, -65536.0]
    assert got[5] == 0.0 and np.signbit(got[5])                           # -0.0 stays -0.0
    assert got[6] == np.float32(1e-40) and got[6] > 0                     # a subnormal is not flushed
    assert got[7] == 65536.0


# the designs whose passband (up to min / 2 - 5 in_rate / P) holds the tone: all but the two strong decimations, where
# 0.02 x the input rate lies in the transition band -- the four ratios of the loop test are among them
TONE_DESIGNS = [d for d in DESIGNS if 0.02 * d[0] <= min(d[0], d[1]) / 2.0 - 5.0 * d[0] / d[2]]
assert len(TONE_DESIGNS) == 8 and {(32_000, 48_000, 32), (50_000, 48_000, 32), (1_000, 750, 32), (50_000, 44_100, 32)} <= set(TONE_DESIGNS)


@pytest.mark.parametrize("in_rate, out_rate, P", TONE_DESIGNS)
def test_a_tone_comes_out_delayed(in_rate, out_rate, P):
    """A tone at 0.02 x the input rate comes out as the ideal sine delayed by the group delay (L P - 1) / 2 samples at L x
    the input rate, within 1e-3 (the -60 dB passband condition; found here: 1.7e-5 to 6e-5), behind the first
    ceil(P L / M) + 1 outputs.  Output m sits at input time m M / L."""
    taps, L, M = resamp_np.design(in_rate, out_rate, P)
    n = 600
    x = np.sin(2 * np.pi * 0.02 * np.arange(n, dtype=np.float64)).astype(np.float32)
    bank = resamp_np.Bank(1, L, M, taps)
    y = np.concatenate([bank.push(x[None, :250])[0], bank.push(x[None, 250:])[0]])
    m = np.arange(y.size, dtype=np.float64)
    ideal = np.sin(2 * np.pi * 0.02 * (m * M / L - (L * P - 1) / 2.0 / L))
    skip = -(-P * L // M) + 1
    err = np.abs(y[skip:] - ideal[skip:]).max()
    print("%d -> %d, P %d: %d outputs, largest error %.3g" % (in_rate, out_rate, P, y.size - skip, err))
    assert y.size - skip > 50
    assert err <= 1e-3
