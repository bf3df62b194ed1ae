#!/usr/bin/env python3
"""Generates the committed golden fixtures.  Run in the build container (where
/root/reference exists): `python tests/golden/make_golden.py`.

  demod_reference.npz   inputs + outputs of the REAL reference Demodulator
                        (dsp/demodulator.cxx driven through DspSource::run by
                        oracle/ref_harness.cxx), all four modes, 8 blocks of 512 frames.
  dspblock_traces.json  scheduling traces of the REAL reference DspBlock runtime
                        (dsp/dspblock.cxx) for the scenarios of oracle/ref_harness.cxx.
  demod_live_cases.npz  the same Demodulator's outputs for the seeded inputs of
                        tests/test_oracle_vs_reference.py (demod_live_inputs below): every
                        mode at 1024-frame blocks, and AM switched to FM after three
                        512-frame blocks (`python tests/golden/make_golden.py live`).
(r01-r04 also wrote oracle_selfcheck_c1.npz here -- the ORACLE's outputs for BASELINE config 1's capture, a
self-check.  r05: the capture goes through the REAL reference chain instead, on the GPU box:
tests/golden/make_c1_reference_golden.py -> reference_c1.npz; the capture itself is synth.rtl_u8_stream(4 * 16384).)
Only data is written; no reference source text is stored.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import wr_oracle as o  # noqa: E402
from webradio_amd import synth  # noqa: E402


MODES = ("AM", "FM", "USB", "LSB")


def demod_live_inputs():
    """The inputs of the live-reference demodulator tests: {mode: iq} at 1024-frame blocks, and the block
    stream that switches from AM to FM."""
    cases = {}
    for i, m in enumerate(MODES):
        rng = np.random.default_rng(10 + i)
        iq = rng.standard_normal(2 * 8192).astype(np.float32)
        iq[:20] = 0.0                       # signed-zero atan2f cases at the start
        iq[40:44] = [-0.0, 1.0, 0.0, -1.0]
        cases[m] = iq
    switch = np.random.default_rng(99).standard_normal(2 * 4096).astype(np.float32)
    return cases, switch


def write_demod_live_cases():
    cases, switch = demod_live_inputs()
    out = {"out_" + m: o.ref_demod(m, iq, 1024) for m, iq in cases.items()}
    out["out_AM_then_FM"] = o.ref_demod("AM", switch, 512, switch_at=3, mode2="FM")
    np.savez_compressed(os.path.join(HERE, "demod_live_cases.npz"), **out)


def main():
    R = o.ref()
    if R is None:
        print("no /root/reference: nothing generated")
        return 1
    if sys.argv[1:] == ["live"]:
        write_demod_live_cases()
        print("demod_live_cases.npz written to", HERE)
        return 0
    rng = np.random.default_rng(20260928)
    iq = rng.standard_normal(2 * 4096).astype(np.float32)
    iq[:16] = 0.0
    iq[32:36] = [-0.0, 1.0, 0.0, -1.0]
    out = {"iq": iq}
    for m in MODES:
        out["out_" + m] = o.ref_demod(m, iq, 512)
    np.savez_compressed(os.path.join(HERE, "demod_reference.npz"), **out)

    traces = [o.harness_trace(R, i) for i in range(R.wr_harness_scenarios())]
    json.dump(traces, open(os.path.join(HERE, "dspblock_traces.json"), "w"), indent=0)
    write_demod_live_cases()

    print("golden fixtures written to", HERE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
