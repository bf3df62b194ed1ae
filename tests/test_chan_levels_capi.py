"""wr_tuner_chan_levels / wr_iq_levels without a GPU: the header and the binding carry them with the same argument
counts, NULL handles are refused with a message, and the numpy restatement of the summation rule the GPU tests compare
bits with (tests/levels_np.py) is held to float64 here first."""
import numpy as np
import pytest

import capicases
import levels_np
from webradio_amd import capi


@pytest.mark.parametrize("name, nargs", [("wr_tuner_chan_levels", 7), ("wr_iq_levels", 5)])
def test_declared_and_bound_with_the_same_arguments(name, nargs):
    capicases.declared_and_bound(name, nargs)


def test_header_says_the_rule_and_cites_the_reference():
    text = capicases.header()
    assert "Added to 6 later: wr_tuner_chan_levels, wr_iq_levels" in text
    for word in ("runs of 16", "groups of 16 runs", "web/receiverhandler.cxx:112,118-119", "dsp/demodulator.cxx:77-115"):
        assert word in text, word


def test_null_handles_are_refused():
    lib = capi.load()
    out = np.zeros(64, np.float32)
    assert lib.wr_tuner_chan_levels(None, capi.ptr(out), None, None, None, None, None) == capi.WR_ERR_ARG
    assert b"wr_tuner_chan_levels" in lib.wr_last_error()
    assert lib.wr_iq_levels(None, capi.ptr(out), 8, None, None) == capi.WR_ERR_ARG
    assert b"wr_iq_levels" in lib.wr_last_error()


@pytest.mark.parametrize("k1", [1, 10, 15, 16, 17, 255, 256, 257, 600, 4097, 100_000])
def test_the_restatement_against_float64(k1):
    rng = np.random.default_rng(k1)
    iq = (rng.standard_normal(2 * k1) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32)
    mean, peak = levels_np.levels(iq)
    assert mean.dtype == np.float32 and peak.dtype == np.float32
    want = levels_np.mean_f64(iq)
    assert want > 0.0
    assert abs(float(mean) - want) <= levels_np.mean_bound(k1) * want
    assert peak == levels_np.power(iq).max()


def test_the_restatement_is_the_rule_spelled_out():
    """the vectorised helper against the rule written as three plain loops"""
    for k1 in (1, 16, 17, 257, 600):
        iq = np.random.default_rng(100 + k1).standard_normal(2 * k1).astype(np.float32)
        e = levels_np.power(iq)
        runs = []
        for j in range(0, k1, 16):
            r = e[j]
            for x in e[j + 1: j + 16]:
                r = np.float32(r + x)
            runs.append(r)
        groups = []
        for h in range(0, len(runs), 16):
            c = runs[h]
            for x in runs[h + 1: h + 16]:
                c = np.float32(c + x)
            groups.append(c)
        s = groups[0]
        for x in groups[1:]:
            s = np.float32(s + x)
        want = np.float32(s / np.float32(k1))
        assert levels_np.bits(levels_np.levels(iq)[0]) == levels_np.bits(want)
