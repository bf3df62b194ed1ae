"""Pins the oracle to the REAL reference where the reference builds from its own sources
(dsp/dspblock.cxx + dsp/demodulator.cxx -> oracle/_ref/libwr_ref.so), live and through
the golden fixtures that were generated from it (tests/golden/make_golden.py).  The live
cases' reference outputs are committed too (demod_live_cases.npz): the oracle is held to
them everywhere, and where _ref is built the reference must still produce them."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ["AM", "FM", "USB", "LSB"]


def _need_ref(oracle):
    if oracle.ref() is None:
        pytest.skip("oracle/_ref not built and /root/reference absent")


@pytest.fixture(scope="module")
def live_cases():
    """(inputs, committed reference outputs) of the live cases; make_golden.py defines the inputs."""
    sys.path.insert(0, GOLDEN)
    from make_golden import demod_live_inputs
    return demod_live_inputs(), np.load(os.path.join(GOLDEN, "demod_live_cases.npz"))


@pytest.mark.parametrize("mode", MODES)
def test_demod_bit_exact_vs_live_reference(oracle, live_cases, mode):
    (cases, _), gold = live_cases
    iq, want = cases[mode], gold["out_" + mode]
    if oracle.ref() is not None:
        assert np.array_equal(oracle.ref_demod(mode, iq, 1024).view(np.uint32), want.view(np.uint32))
    got, _ = oracle.demod(MODES.index(mode), (0.0, 0.0), iq)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32))


def test_demod_state_carries_across_blocks_and_mode_switch(oracle, live_cases):
    (_, iq), gold = live_cases
    want = gold["out_AM_then_FM"]
    if oracle.ref() is not None:
        assert np.array_equal(oracle.ref_demod("AM", iq, 512, switch_at=3, mode2="FM"), want)
    a, prev = oracle.demod(oracle.AM, (0.0, 0.0), iq[: 2 * 1536])
    b, _ = oracle.demod(oracle.FM, prev, iq[2 * 1536:])
    assert np.array_equal(want, np.concatenate([a, b]))


@pytest.mark.parametrize("mode", MODES)
def test_demod_golden_fixture(oracle, mode):
    """Committed vectors produced by the reference's own Demodulator (no _ref needed)."""
    g = np.load(os.path.join(GOLDEN, "demod_reference.npz"))
    got, _ = oracle.demod(MODES.index(mode), (0.0, 0.0), g["iq"])
    assert np.array_equal(got.view(np.uint32), g["out_" + mode].view(np.uint32))


def test_dspblock_trace_golden(oracle):
    """The DspBlock scheduling traces of the real reference are committed; when _ref is
    available they must still be what it produces."""
    _need_ref(oracle)
    import json
    gold = json.load(open(os.path.join(GOLDEN, "dspblock_traces.json")))
    R = oracle.ref()
    assert R.wr_harness_scenarios() == len(gold)
    for i, want in enumerate(gold):
        assert oracle.harness_trace(R, i) == want
