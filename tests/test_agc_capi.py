"""The AGC without a GPU: the five functions are declared and bound with the same argument counts, the header carries
the rule, NULL handles are refused by name, wr_agc_design's numbers are numpy's, and the restatement the GPU tests
compare bits with (tests/agc_np.py) is held to the rule's plain loop and to the rule's two promises here first."""
import ctypes as C

import numpy as np
import pytest

import capicases
import agc_np
from webradio_amd import capi

STEPS = [0, 1, 2787, 1 << 23, 1 << 31]


@pytest.mark.parametrize("name, nargs", [("wr_agc_design", 7), ("wr_agc_rows", 9), ("wr_chan_set_agc", 6),
                                         ("wr_chan_get_agc", 7), ("wr_tuner_agc_info", 3)])
def test_declared_and_bound_with_the_same_arguments(name, nargs):
    capicases.declared_and_bound(name, nargs)


def test_header_says_the_rule():
    text = capicases.header()
    assert "Added to 6 later: wr_agc_design, wr_agc_rows, wr_chan_set_agc, wr_chan_get_agc, wr_tuner_agc_info" in text
    for word in ("0x7f7fffff", "E[m]   = max(L[m], E[m-1] - step, floor)", "g[m]   = target / env[m]", "prefix",
                 "audio filter -> squelch -> AGC -> af_gain -> scale", "0.72 and 1.44", "leaves every bit as it was",
                 "dsp/demodulator.cxx:88-104", "io/tuner.h:56-62"):
        assert word in text, word


def test_null_handles_are_refused():
    lib = capi.load()
    a = np.zeros(4, np.float32)
    u = np.zeros(4, np.uint32)
    assert lib.wr_agc_rows(None, capi.ptr(a), 4, 1, 4, capi.ptr(a), capi.ptr(u), capi.ptr(u), capi.ptr(u)) == capi.WR_ERR_ARG
    assert b"wr_agc_rows" in lib.wr_last_error()
    assert lib.wr_chan_set_agc(None, 0, C.c_float(-12.0), C.c_float(20.0), C.c_float(60.0), 1) == capi.WR_ERR_ARG
    assert b"wr_chan_set_agc" in lib.wr_last_error()
    assert lib.wr_chan_get_agc(None, 0, None, None, None, None, None) == capi.WR_ERR_ARG
    assert b"wr_chan_get_agc" in lib.wr_last_error()
    assert lib.wr_tuner_agc_info(None, None, None) == capi.WR_ERR_ARG
    assert b"wr_tuner_agc_info" in lib.wr_last_error()
    assert lib.wr_agc_design(C.c_float(-12.0), C.c_float(20.0), C.c_float(60.0), 10_000, None, None, None) == capi.WR_ERR_ARG
    assert b"wr_agc_design" in lib.wr_last_error()


def _design(target_dbfs, decay, max_gain, rate):
    t, f, s = C.c_float(), C.c_uint(), C.c_uint()
    rc = capi.load().wr_agc_design(C.c_float(target_dbfs), C.c_float(decay), C.c_float(max_gain), rate, C.byref(t),
                                   C.byref(f), C.byref(s))
    return rc, np.float32(t.value), f.value, s.value


def test_design_twenty_db_per_second_at_ten_kilohertz():
    rc, target, floor_bits, step = _design(-12.0, 20.0, 60.0, 10_000)
    assert rc == capi.WR_OK and step == 2787


@pytest.mark.parametrize("args", [(-12.0, 20.0, 60.0, 10_000), (-3.5, 7.25, 33.0, 8_000), (-100.0, 1.0e4, 120.0, 1),
                                  (0.0, 0.0, 0.0, 48_000)])
def test_design_equals_numpy(args):
    rc, target, floor_bits, step = _design(*args)
    assert rc == capi.WR_OK
    wt, wf, ws = agc_np.design(*args)
    assert agc_np.bits(target)[0] == agc_np.bits(wt)[0]
    assert floor_bits == wf and step == ws
    assert 0x00800000 <= floor_bits <= 0x7F7FFFFF and step <= 1 << 31
    if args[1] == 0.0:
        assert step == 0
    if args == (-100.0, 1.0e4, 120.0, 1):
        assert step == 1 << 31                      # clamped


@pytest.mark.parametrize("args", [(float("nan"), 20.0, 60.0, 10_000), (-12.0, float("nan"), 60.0, 10_000),
                                  (-12.0, 20.0, float("nan"), 10_000), (0.5, 20.0, 60.0, 10_000),
                                  (-100.5, 20.0, 60.0, 10_000), (-12.0, -1.0, 60.0, 10_000), (-12.0, 10_001.0, 60.0, 10_000),
                                  (-12.0, 20.0, -0.5, 10_000), (-12.0, 20.0, 120.5, 10_000), (-12.0, 20.0, 60.0, 0)])
def test_design_refuses(args):
    rc, *_ = _design(*args)
    assert rc == capi.WR_ERR_ARG
    assert b"wr_agc_design" in capi.load().wr_last_error()


def _row(n, seed):
    """bursts decades apart, runs of exact zeros, negative values; no denormals"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, 1, n)).astype(np.float32)
    v[rng.random(n) < 0.2] = 0.0
    if n > 40:
        v[n // 3: n // 3 + 17] = 0.0
    assert not np.any((v != 0) & (np.abs(v) < np.finfo(np.float32).tiny))
    return v


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_the_closed_form_is_the_loop(n, step):
    v = _row(n, n + 7)
    _, floor_bits, _ = agc_np.design(-12.0, 20.0, 60.0, 10_000)
    want, wlast = agc_np.envelope_loop(v, floor_bits, step, floor_bits)
    got, glast = agc_np.envelope(v, floor_bits, step, floor_bits)
    assert np.array_equal(got, want) and glast == wlast
    # ... also with the row split at uneven edges and the carry passed on
    state, parts = floor_bits, []
    edges = sorted({0, n} | {e for e in (1, 7, 64, 1031, 2500) if e < n})
    for a, b in zip(edges[:-1], edges[1:]):
        e, state = agc_np.envelope(v[a:b], floor_bits, step, state)
        parts.append(e)
    assert np.array_equal(np.concatenate(parts), want) and state == wlast


@pytest.mark.parametrize("step", STEPS)
def test_the_two_promises(step):
    """instant attack: |out| <= target up to the two roundings; the gain never exceeds target / floor"""
    v = _row(5000, 99)
    target, floor_bits, _ = agc_np.design(-12.0, 20.0, 60.0, 10_000)
    out, _ = agc_np.apply(v, target, floor_bits, step, floor_bits)
    assert float(np.abs(out).max()) <= float(target) * (1.0 + 2e-7)
    e, _ = agc_np.envelope(v, floor_bits, step, floor_bits)
    g = np.float32(target) / e.view(np.float32)
    gmax = np.float32(target) / np.array([floor_bits], np.uint32).view(np.float32)[0]
    assert float(g.max()) <= float(gmax)
    assert np.all(e.view(np.float32) >= np.abs(v))
