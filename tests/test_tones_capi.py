"""The tone bank without a GPU: the seven functions are declared and bound with the same argument counts, the header
carries the rule, NULL handles are refused by name, wr_tone_step's numbers are numpy's, and the restatement the GPU tests
compare bits with (tests/tones_np.py) is held here first to the rule written as plain loops (bit for bit), to a float64 DFT
at the exact phase (within a bound derived below), and to the detection conditions on audio from the oracle chain."""
import ctypes as C
import re

import numpy as np
import pytest

import capicases
import tones_np
from webradio_amd import CTCSS_HZ, capi

NAMES = [("wr_tone_step", 3), ("wr_tones_create", 6), ("wr_tones_destroy", 1), ("wr_tones_reset", 2),
         ("wr_tones_push_rows", 5), ("wr_tuner_tones_push", 3), ("wr_tones_read", 6)]
WINDOWS = [16, 17, 500]
SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, -0.0, 1e-40, 64.0]


@pytest.mark.parametrize("name, nargs", NAMES)
def test_declared_and_bound_with_the_same_arguments(name, nargs):
    capicases.declared_and_bound(name, nargs)


def test_header_says_the_rule():
    text = capicases.header()
    assert re.search(r"#define\s+WR_ABI_VERSION\s+6\b", text)
    assert re.search(r"Added to 6 later: wr_tone_step, wr_tones_create, wr_tones_destroy, wr_tones_reset,\s+"
                     r"wr_tones_push_rows, wr_tuner_tones_push, wr_tones_read\.", text)
    for word in ("v'   = 0.0f if (bits(v) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else v",
                 "w    = min(max(v', -64.0f), 64.0f) * 16777216.0f", "p    = (uint32)(j * step_t)", "i    = p >> 20",
                 "s    = T12[i],  c = T12[(i + 1024) & 4095]", "T12[i] = wr_sin_table()[16 * i]",
                 "I_t += (int64) rint(w * c)      Q_t += (int64) rint(w * s)",
                 "qv   = (int64) rint(w)          E  += (qv * qv) >> 14",
                 "rho_t = 2 (I_t^2 + Q_t^2) / (W * E * 2^14)", "wr_tuner_seek, wr_chan_reset_history or a retune",
                 "rho does not depend on af_gain and scale", "muting audio by tone", "host-side C++ class",
                 "window functions other than", "per-receiver tone lists", "time sharding"):
        assert word in text, word


def test_null_handles_are_refused():
    lib = capi.load()
    a = np.zeros(4, np.float32)
    u = np.ones(4, np.uint32)
    h = C.c_void_p()
    for call, name in ((lambda: lib.wr_tones_create(C.byref(h), None, 1, capi.ptr(u), 1, 16), b"wr_tones_create"),
                       (lambda: lib.wr_tones_create(None, None, 1, capi.ptr(u), 1, 16), b"wr_tones_create"),
                       (lambda: lib.wr_tones_reset(None, -1), b"wr_tones_reset"),
                       (lambda: lib.wr_tones_push_rows(None, capi.ptr(a), 4, 1, 4), b"wr_tones_push_rows"),
                       (lambda: lib.wr_tuner_tones_push(None, None, None), b"wr_tuner_tones_push"),
                       (lambda: lib.wr_tones_read(None, capi.ptr(a), None, None, None, None), b"wr_tones_read"),
                       (lambda: lib.wr_tone_step(C.c_double(100.0), 1000, None), b"wr_tone_step")):
        assert call() == capi.WR_ERR_ARG, name
        assert name in lib.wr_last_error(), (name, lib.wr_last_error())
    assert lib.wr_tones_destroy(None) == capi.WR_OK                    # as wr_spectrum_destroy: nothing to do


def _step(hz, rate):
    s = C.c_uint(0xDEADBEEF)
    return capi.load().wr_tone_step(C.c_double(hz), rate, C.byref(s)), s.value


@pytest.mark.parametrize("rate", [1_000, 8_000, 10_000, 48_000])
def test_tone_step_equals_numpy(rate):
    for hz in CTCSS_HZ:
        rc, step = _step(hz, rate)
        assert rc == capi.WR_OK
        assert step == tones_np.step_of(hz, rate), hz
        assert 0 < step < 1 << 31


def test_ctcss_list():
    assert len(CTCSS_HZ) == 50 and list(CTCSS_HZ) == sorted(set(CTCSS_HZ))
    assert CTCSS_HZ[0] == 67.0 and CTCSS_HZ[-1] == 254.1 and 100.0 in CTCSS_HZ and 151.4 in CTCSS_HZ


@pytest.mark.parametrize("hz, rate", [(0.0, 1000), (500.0, 1000), (24_000.0, 48_000), (float("nan"), 1000), (-67.0, 1000),
                                      (600.0, 1000), (67.0, 0)])
def test_tone_step_refuses(hz, rate):
    rc, _ = _step(hz, rate)
    assert rc == capi.WR_ERR_ARG
    assert b"wr_tone_step" in capi.load().wr_last_error()


# ---- the restatement against the rule as plain loops ---------------------------------------------------------------------------

def _loop_bank(v, steps, W):
    """the header's lines, one frame and one tone at a time; returns what wr_tones_read would: (iq, E, windows, fill)"""
    t12 = tones_np.table12()
    f32 = np.float32
    I, Q, E = [0] * len(steps), [0] * len(steps), 0
    lat, lat_e, windows, j = [[0, 0] for _ in steps], 0, 0, 0
    for x in np.asarray(v, np.float32):
        bits = int(np.array([x], np.float32).view(np.uint32)[0])
        vv = f32(0.0) if (bits & 0x7FFFFFFF) >= 0x7F800000 else x
        w = f32(min(max(vv, f32(-64.0)), f32(64.0))) * f32(16777216.0)
        assert abs(float(w)) <= 2.0 ** 30
        for t, step in enumerate(steps):
            p = (j * int(step)) & 0xFFFFFFFF
            i = p >> 20
            s, c = t12[i], t12[(i + 1024) & 4095]
            I[t] += int(np.rint(f32(w * c)))
            Q[t] += int(np.rint(f32(w * s)))
        qv = int(np.rint(w))
        E += (qv * qv) >> 14
        j += 1
        if j == W:
            lat, lat_e = [[a, b] for a, b in zip(I, Q)], E
            windows += 1
            I, Q, E, j = [0] * len(steps), [0] * len(steps), 0, 0
    return np.array(lat, np.int64), lat_e, windows, j


@pytest.mark.parametrize("W", WINDOWS)
def test_the_restatement_is_the_loop(W):
    steps = [tones_np.step_of(67.0, 1000), tones_np.step_of(254.1, 1000), (1 << 31) - 1, 1]
    n = 3 * W + W // 3 + 1
    v = capicases.audio(n, W, SPECIAL, 3)
    # checked after every push of an uneven cut: a push of one frame, several pushes per window, one that ends exactly on
    # a window end, one with two window ends and two frames behind them
    cuts = [1, W // 2, W, 3 * W + 2, n]
    bank = tones_np.Bank(1, steps, W)
    pos = 0
    for c in cuts:
        bank.push(v[pos:c][None, :])
        pos = c
        iq, e, windows, fill = _loop_bank(v[:c], steps, W)
        assert np.array_equal(bank.iq[0], iq), (W, c)
        assert int(bank.energy[0]) == e and int(bank.windows[0]) == windows and int(bank.fill[0]) == fill, (W, c)
    assert int(bank.windows[0]) == 3 and int(bank.fill[0]) == n - 3 * W


def test_special_values_count_as_the_rule_says():
    w = tones_np.quantise(np.array(SPECIAL, np.float32))
    assert list(w[:6]) == [0.0, 0.0, 0.0, 2.0 ** 30, -(2.0 ** 30), 0.0]
    assert w[6] == np.float32(1e-40) * np.float32(16777216.0) and w[6] > 0       # a subnormal is not flushed
    assert w[7] == 2.0 ** 30
    _, _, E = tones_np.sums(np.full(16, 64.0, np.float32), [1 << 28], 0)
    assert E == 16 << 46                                                          # 2^46 per frame at the clamp


# ---- the restatement against a float64 DFT -------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINDOWS)
def test_against_a_float64_dft(W):
    """Per window, with X64 = sum_j v'_j exp(-i theta_j) and theta_j = 2 pi (j step mod 2^32) / 2^32 -- the exact phase --

        |I - 2^24 Re X64|, |Q + 2^24 Im X64|  <=  2^24 (2 pi / 4096 + 2^-22) sum |v'| + W

    DERIVED, not tuned: the table is read at the phase with its low 20 bits cut off, an error below 2 pi / 4096 in the
    angle and so in cos and sin (their slope is at most 1); the table's float32 entries and the float32 product add a few
    2^-24 relative to |w|, counted as 2^-22; each rint moves a term by at most half a unit, W / 2 in all, counted as W."""
    steps = np.array([tones_np.step_of(hz, 1000) for hz in (67.0, 100.0, 254.1, 499.9)], np.uint64)
    v = capicases.audio(W, 100 + W, None, 3)
    I, Q, _ = tones_np.sums(v, steps, 0)
    vc = tones_np.clean(v).astype(np.float64)
    j = np.arange(W, dtype=np.uint64)
    theta = 2.0 * np.pi * ((j[:, None] * steps[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0
    re = (vc[:, None] * np.cos(theta)).sum(axis=0)
    im = (vc[:, None] * np.sin(theta)).sum(axis=0)
    bound = 2.0 ** 24 * (2.0 * np.pi / 4096.0 + 2.0 ** -22) * np.abs(vc).sum() + W
    err_i = np.abs(I.astype(np.float64) - 2.0 ** 24 * re)
    err_q = np.abs(Q.astype(np.float64) - 2.0 ** 24 * im)
    print("W %d: largest |I - 2^24 Re X| %.4g, |Q + 2^24 Im X| %.4g, bound %.4g" % (W, err_i.max(), err_q.max(), bound))
    assert np.all(err_i <= bound) and np.all(err_q <= bound)


def test_a_pure_tone_has_rho_one():
    W, rate = 500, 1000
    steps = [tones_np.step_of(hz, rate) for hz in CTCSS_HZ]
    for hz in (67.0, 100.0, 254.1):
        v = (0.05 * np.sin(2 * np.pi * hz * np.arange(W) / rate + 0.3)).astype(np.float32)
        bank = tones_np.Bank(1, steps, W)
        bank.push(v[None, :])
        rho = tones_np.ratios(bank.iq, bank.energy, W)[0]
        own = CTCSS_HZ.index(hz)
        # (a real tone's mirror image at -hz leaks 1 / (2 pi hz W / rate) of its amplitude at most: 0.5 % at 67 Hz, so
        # 1 % of the power; the phase quantisation and the rounding are far below that)
        assert 0.98 <= rho[own] <= 1.02, (hz, rho[own])
        # the nearest neighbours, 2.3 to 2.6 Hz away, get |sinc(df * 0.5)| <= 0.2 of the amplitude plus the mirror image's
        # 0.5 % at most: (0.2 + 0.01)^2
        assert np.delete(rho, own).max() <= 0.0441, hz


# ---- the detection conditions on the oracle chain ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_rho(oracle):
    """rho[5][50] of the first window of 500 audio frames of tones_np's five FM receivers, through the oracle's chain"""
    rx = [oracle.Receiver(tones_np.FS, f, tones_np.CHAN_PASSBAND, tones_np.CHAN_RATE, capi.WR_FM, tones_np.AUDIO_PASSBAND,
                          tones_np.AUDIO_RATE) for f in tones_np.IFS]
    bank = tones_np.Bank(len(rx), [tones_np.step_of(hz, tones_np.AUDIO_RATE) for hz in CTCSS_HZ], 500)
    for b in range(10):
        iq = tones_np.fm_block(100_000, b * 100_000)
        bank.push(np.stack([x.run(iq)[0] for x in rx]))
    assert list(bank.windows) == [1] * 5 and list(bank.fill) == [0] * 5
    return tones_np.ratios(bank.iq, bank.energy, 500)


def test_detection_on_the_oracle_chain(oracle_rho):
    margins, untoned = tones_np.detection(oracle_rho, CTCSS_HZ)
    print("oracle: own-tone rho %s; own / largest other %s; untoned largest / smallest own %.4g" % (
        ["%.4f" % oracle_rho[r, CTCSS_HZ.index(hz)] for r, hz in enumerate(tones_np.TONED)], ["%.1f" % m for m in margins],
        untoned))
    assert min(margins) >= 4.0
    assert untoned < 0.25
    # ... with room: the deviations were chosen so that the oracle alone clears both by a factor of four and more
    assert min(margins) >= 16.0 and untoned < 0.0625
