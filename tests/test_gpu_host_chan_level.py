"""-m gpu: Demodulator::inputLevel() through the host runtime (tests/cxx/chan_level.cxx): a FileTuner recording feeds
three Receivers, each asked for its level after every block.

Inside the tuner batch the three answers of a block come out of ONE wr_tuner_chan_levels call; block by block
(WEBRADIO_NO_FUSION=1) each Demodulator measures its own input with wr_iq_levels from the block after its first call on.
Both are the same rule of summation over the same frames, and with WEBRADIO_NCO=exact the channel IQ of both runs is the
same bit for bit, so the dB values are the same bits."""
import json
import math
import os

import numpy as np
import pytest

import _proc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "webradio_amd", "host")
LIB = os.path.join(ROOT, "webradio_amd", "lib")
FS, BLOCK, BLOCKS = 2_400_000, 15_000, 4
IFS = (-300_000, 100_000, 500_000)
AMP = 0.25


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """compiled with the flags tests/cxx/Makefile gives host_bench (the rpaths absolute: the program lies elsewhere)"""
    exe = str(tmp_path_factory.mktemp("chan_level") / "chan_level")
    _proc.run(["g++", "-std=c++11", "-O2", "-Wall", "-fPIC", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-fPIE",
               os.path.join(ROOT, "tests", "cxx", "chan_level.cxx"), "-o", exe, "-L" + HOST, "-lwebradio_host",
               "-L" + LIB, "-lwebradio_amd", "-Wl,-rpath," + HOST, "-Wl,-rpath," + LIB, "-lm"], timeout=300)
    return exe


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """three FM carriers of amplitude 0.25, one per receiver, in the RTL-SDR byte format (rtlsdrtuner.cxx:106)"""
    from webradio_amd import synth
    x = synth.fm_stream(BLOCK * BLOCKS, FS, IFS, amp=AMP, beta=2.0, fm_base=3000.0, fm_step=500.0, noise_dbfs=-40, seed=11)
    raw = np.clip(np.round(127.5 + 127.0 * x.astype(np.float64)), 0, 255).astype(np.uint8)
    path = str(tmp_path_factory.mktemp("recording") / "capture.u8")
    raw.tofile(path)
    return path


_runs = {}


@pytest.fixture(scope="module")
def run(program, recording):
    """run(ask, **env) -> the driver's figures, "answers" as an array [block][receiver][answered, mean bits, peak bits];
    every distinct run is made once"""
    def go(ask, **extra):
        key = (ask,) + tuple(sorted(extra.items()))
        if key not in _runs:
            env = dict(os.environ, WEBRADIO_QUIET="1")
            for name in ("WEBRADIO_AUDIO_LATE", "WEBRADIO_NO_FUSION", "WEBRADIO_NCO", "WEBRADIO_NCO_EXACT", "WEBRADIO_PIECES"):
                env.pop(name, None)
            env.update(extra)
            text = _proc.output([program, recording, str(FS), str(BLOCK), str(BLOCKS), "1" if ask else "0"] + [str(f) for f in IFS],
                                timeout=120, env=env).decode()
            info = json.loads(text.strip().splitlines()[-1])
            assert info["audio_samples"] == BLOCKS * BLOCK // 50
            if ask:
                info["answers"] = np.array(info["answers"], np.int64).reshape(BLOCKS, len(IFS), 3)
            _runs[key] = info
        return _runs[key]
    yield go
    _runs.clear()


def _db(bits):
    return np.asarray(bits, np.int64).astype(np.uint32).view(np.float32)


def test_one_call_per_block_serves_every_receiver(run):
    info = run(True, WEBRADIO_NCO="exact", WEBRADIO_PIECES="1")
    assert info["block_kernel_calls"] == 0               # every receiver stayed in the tuner batch
    assert info["level_calls"] == BLOCKS                  # three receivers asked after each block: one call per block
    a = info["answers"]
    assert (a[:, :, 0] == 1).all()
    mean, peak = _db(a[:, :, 1]), _db(a[:, :, 2])
    print("mean dBFS per block and receiver:\n%s\npeak:\n%s" % (mean, peak))
    # a carrier of amplitude 0.25 (-12 dBFS) over noise at -40 dBFS, through a channel filter whose passband gain lies
    # somewhere between 1/8 and 1: between -30 and -12 dBFS; FM has a constant envelope, so the peak is close above the mean
    top = 20.0 * math.log10(AMP)
    assert np.isfinite(mean).all() and (mean > top - 18.0).all() and (mean < top + 0.1).all()
    assert (peak >= mean).all() and (peak < mean + 3.0).all()


def test_fused_against_block_by_block_bit_for_bit(run):
    fused = run(True, WEBRADIO_NCO="exact", WEBRADIO_PIECES="1")
    plain = run(True, WEBRADIO_NCO="exact", WEBRADIO_NO_FUSION="1")
    assert plain["level_calls"] == 0 and plain["block_kernel_calls"] > 0
    a, b = fused["answers"], plain["answers"]
    assert (b[0, :, 0] == 0).all()                        # stand-alone: the first call answers false and asks ...
    assert (b[1:, :, 0] == 1).all()                       # ... and from the next block on there is a measurement
    assert np.array_equal(a[1:, :, 1:], b[1:, :, 1:])     # the same dB values, bit for bit


def test_default_nco_against_exact(run):
    """the project's own 1e-6 bound on ROTATE's channel IQ, turned into power: |z + d|^2 <= |z|^2 (1 + 2 |d| / |z| + ...)
    for a carrier of amplitude a at the filter's output, a from the EXACT run's own level"""
    exact = run(True, WEBRADIO_NCO="exact", WEBRADIO_PIECES="1")
    rotate = run(True, WEBRADIO_PIECES="1")
    assert rotate["block_kernel_calls"] == 0 and rotate["level_calls"] == BLOCKS
    want, got = _db(exact["answers"][:, :, 1]).astype(np.float64), _db(rotate["answers"][:, :, 1]).astype(np.float64)
    a = np.sqrt(10.0 ** (want / 10.0))
    bound = 10.0 * np.log10(1.0 + 2.0 * 1e-6 / a)
    print("ROTATE against EXACT: worst %.3g dB, bound %.3g dB" % (np.abs(got - want).max(), bound.min()))
    assert (np.abs(got - want) <= bound).all()


def test_nobody_asking_costs_nothing(run):
    """block by block a Receiver is four kernels a block (wr_mix, two wr_fir_decimate, wr_demod), as before: no launch
    was added for nobody.  Asked, each Demodulator adds one wr_iq_levels per block from the second block on."""
    quiet = run(False, WEBRADIO_NCO="exact", WEBRADIO_NO_FUSION="1")
    asked = run(True, WEBRADIO_NCO="exact", WEBRADIO_NO_FUSION="1")
    assert quiet["block_kernel_calls"] == 4 * len(IFS) * BLOCKS
    assert asked["block_kernel_calls"] == quiet["block_kernel_calls"] + len(IFS) * (BLOCKS - 1)
    fused = run(False, WEBRADIO_NCO="exact", WEBRADIO_PIECES="1")
    assert fused["block_kernel_calls"] == 0 and fused["level_calls"] == 0
