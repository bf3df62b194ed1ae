"""-m gpu: a receiver's audio spectrum through the host runtime (webradio_amd/host/spectrumsink.cxx with one input
channel -- the reference's FIXMEs at io/spectrumsink.cxx:62-64): tests/cxx/audio_spectrum.cxx connects a SpectrumSink and
the retaining AudioStreamManager behind a Receiver's audio filter, and the sink's row is held to the oracle's spectrum
of the last complete frame of the audio the receiver delivered, as (x, 0), with the project's DB_ATOL."""
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
FS, BLOCK, BLOCKS, IF_HZ, FFT = 2_400_000, 15_000, 4, 100_000, 256      # 300 audio frames a block: frames straddle blocks


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """compiled with the flags tests/cxx/Makefile gives host_bench (the rpaths absolute: the program lies elsewhere)"""
    exe = str(tmp_path_factory.mktemp("audio_spectrum") / "audio_spectrum")
    _proc.run(["g++", "-std=c++11", "-O2", "-Wall", "-fPIC", "-I" + HOST, "-I" + os.path.join(ROOT, "include"), "-fPIE",
               os.path.join(ROOT, "tests", "cxx", "audio_spectrum.cxx"), "-o", exe, "-L" + HOST, "-lwebradio_host",
               "-L" + LIB, "-lwebradio_amd", "-Wl,-rpath," + HOST, "-Wl,-rpath," + LIB, "-lm"], timeout=300)
    return exe


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    from webradio_amd import synth
    raw = synth.rtl_u8_stream(BLOCK * BLOCKS, FS, IF_HZ, tone=3000.0, beta=2.0, seed=11)
    path = str(tmp_path_factory.mktemp("recording") / "capture.u8")
    raw.tofile(path)
    return path, raw


def _strong_close(got, want):
    strong = want >= want.max() - 60.0
    err = float(np.abs(got[strong] - want[strong]).max())
    print("n=%d dB error on strong bins %.3g (bound %.3g)" % (want.size, err, DB_ATOL))
    assert err <= DB_ATOL


def _oracle_row(oracle, iq):
    o = oracle.Spectrum(FFT)
    o.process(np.ascontiguousarray(iq, np.float32))
    assert o.frames_done == 1
    return o.get()


@pytest.mark.parametrize("iq_sink", [0, 1], ids=["audio-sink", "audio-and-tuner-sink"])
def test_audio_spectrum_of_a_receiver(program, recording, oracle, tmp_path, iq_sink):
    path, raw = recording
    out = str(tmp_path / "out")
    env = dict(os.environ, WEBRADIO_QUIET="1")
    env.pop("WEBRADIO_AUDIO_LATE", None)
    info = json.loads(_proc.output([program, path, out, str(FS), str(BLOCK), str(BLOCKS), str(IF_HZ), str(FFT),
                                    str(iq_sink)], timeout=120, env=env).decode().strip().splitlines()[-1])
    assert info["block_kernel_calls"] == 0              # the receiver stayed in the tuner batch
    audio = np.fromfile(out + ".audio", np.float32)
    assert audio.size == info["audio_samples"] == BLOCKS * BLOCK // 50
    assert float(np.abs(audio).max()) > 0.0
    done = audio.size // FFT                            # the sink's most recent complete frame
    frame = audio[(done - 1) * FFT: done * FFT]
    x0 = np.zeros(2 * FFT, np.float32)
    x0[0::2] = frame
    row = np.fromfile(out + ".row", np.float32)
    assert row.size == FFT
    _strong_close(row, _oracle_row(oracle, x0))
    assert np.array_equal(row[FFT // 2 + 1:].view(np.uint32), row[1: FFT // 2][::-1].view(np.uint32))
    if iq_sink:
        iq = ((raw.astype(np.float32) - 128.0) / 128.0).astype(np.float32)       # rtlsdrtuner.cxx:106
        last = (BLOCKS * BLOCK) // FFT
        iqrow = np.fromfile(out + ".iqrow", np.float32)
        _strong_close(iqrow, _oracle_row(oracle, iq[2 * (last - 1) * FFT: 2 * last * FFT]))
