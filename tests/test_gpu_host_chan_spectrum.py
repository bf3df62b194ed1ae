"""-m gpu: a SpectrumSink on every receiver's CHANNEL filter through the host runtime (tests/cxx/chan_spectrum.cxx).

Such sinks no longer throw their receivers out of the tuner batch: they receive no samples, and getSpectrum() is served
by ONE wr_tuner_chan_spectra launch for all of them, the frame being the reference's (webradio_amd/host/spectrumframing.h).
The yardstick is the reference's own dataflow, block by block (WEBRADIO_NO_FUSION=1), where each sink is fed its channel
filter's output: with WEBRADIO_NCO=exact the channel IQ of both runs is the same bit for bit, so the rows may differ by
the two transforms' rounding only -- DB_ATOL on bins within 60 dB of the peak, as everywhere."""
import json
import os

import numpy as np
import pytest

import _proc
from speccases import DB_ATOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "webradio_amd", "host")
LIB = os.path.join(ROOT, "webradio_amd", "lib")
# 750 channel-rate frames per part of a block (two parts): FFT 256 + its hop fit, frames straddle blocks; FFT 512 does not
FS, BLOCK, BLOCKS, FFT = 2_400_000, 15_000, 4, 256
IFS = (-300_000, 100_000, 500_000)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """compiled with the flags tests/cxx/Makefile gives host_bench (the rpaths absolute: the program lies elsewhere)"""
    exe = str(tmp_path_factory.mktemp("chan_spectrum") / "chan_spectrum")
    _proc.run(["g++", "-std=c++11", "-O2", "-Wall", "-fPIC", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-fPIE",
               os.path.join(ROOT, "tests", "cxx", "chan_spectrum.cxx"), "-o", exe, "-L" + HOST, "-lwebradio_host",
               "-L" + LIB, "-lwebradio_amd", "-Wl,-rpath," + HOST, "-Wl,-rpath," + LIB, "-lm"], timeout=300)
    return exe


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """three FM carriers of amplitude 0.25, one per receiver, in the RTL-SDR byte format (rtlsdrtuner.cxx:106)"""
    from webradio_amd import synth
    x = synth.fm_stream(BLOCK * BLOCKS, FS, IFS, amp=0.25, beta=2.0, fm_base=3000.0, fm_step=500.0, noise_dbfs=-40, seed=11)
    raw = np.clip(np.round(127.5 + 127.0 * x.astype(np.float64)), 0, 255).astype(np.uint8)
    path = str(tmp_path_factory.mktemp("recording") / "capture.u8")
    raw.tofile(path)
    return path


_runs = {}


@pytest.fixture(scope="module")
def run(program, recording, tmp_path_factory):
    """run(fft, **env) -> (the driver's figures, rows[receiver][fft]); every distinct run is made once"""
    def go(fft, **extra):
        key = (fft,) + tuple(sorted(extra.items()))
        if key not in _runs:
            out = str(tmp_path_factory.mktemp("run") / "out")
            env = dict(os.environ, WEBRADIO_QUIET="1")
            for name in ("WEBRADIO_AUDIO_LATE", "WEBRADIO_NO_FUSION", "WEBRADIO_NCO", "WEBRADIO_NCO_EXACT", "WEBRADIO_PIECES"):
                env.pop(name, None)
            env.update(extra)
            text = _proc.output([program, recording, out, str(FS), str(BLOCK), str(BLOCKS), str(fft)] + [str(f) for f in IFS],
                                timeout=120, env=env).decode()
            info = json.loads(text.strip().splitlines()[-1])
            rows = np.fromfile(out + ".rows", np.float32).reshape(len(IFS), fft)
            assert info["audio_samples"] == BLOCKS * BLOCK // 50
            _runs[key] = (info, rows)
        return _runs[key]
    yield go
    _runs.clear()


def _close(got, want, within_db, what):
    worst = 0.0
    for r in range(want.shape[0]):
        assert np.isfinite(want[r]).all() and want[r].max() > -60.0         # (a carrier: the row was filled)
        strong = want[r] >= want[r].max() - within_db
        worst = max(worst, float(np.abs(got[r][strong] - want[r][strong]).max()))
    print("%s: dB error on bins within %.0f dB of the peak %.3g (bound %.3g)" % (what, within_db, worst, DB_ATOL))
    assert worst <= DB_ATOL


def test_tapped_receivers_stay_in_the_batch(run):
    info, rows = run(FFT)
    assert info["block_kernel_calls"] == 0              # every receiver stayed in the tuner batch
    assert info["spectra_calls"] == 1                   # three sinks read after the same block: one launch, one copy
    assert (rows != -1.0).any(axis=1).all()


def test_exact_nco_against_the_reference_dataflow(run):
    fused, rows = run(FFT, WEBRADIO_NCO="exact")
    plain, want = run(FFT, WEBRADIO_NCO="exact", WEBRADIO_NO_FUSION="1")
    assert fused["block_kernel_calls"] == 0 and fused["spectra_calls"] == 1
    assert plain["block_kernel_calls"] > 0 and plain["spectra_calls"] == 0
    _close(rows, want, 60.0, "fused, exact NCO, against block by block")


def test_default_nco_against_the_exact_rows(run):
    """ROTATE's channel IQ is within 1e-6 of the exact mode's (the project's own bound); taken coherently over 256 windowed
    samples against a carrier of amplitude >= 0.2 that is below 0.02 dB on a bin 40 dB under the peak"""
    _, rows = run(FFT)
    _, want = run(FFT, WEBRADIO_NCO="exact")
    _close(rows, want, 40.0, "fused, ROTATE, against fused exact")


def test_a_sink_whose_frames_do_not_fit_keeps_the_reference_dataflow(run):
    """FFT 512: 1024 > 750 channel frames per part -- the receivers run block by block, as before, and the rows are the
    block-by-block run's"""
    unfused, rows = run(512, WEBRADIO_NCO="exact")
    plain, want = run(512, WEBRADIO_NCO="exact", WEBRADIO_NO_FUSION="1")
    assert unfused["block_kernel_calls"] > 0 and unfused["spectra_calls"] == 0
    assert plain["block_kernel_calls"] > 0
    _close(rows, want, 60.0, "not tapped")
