"""-m gpu: wr_tuner_chan_spectra -- the CHANNEL spectrum of every receiver of a tuner from one launch (a SpectrumSink on
each Receiver's channel filter, io/spectrumsink.cxx:88-142 behind radio.cxx:68-76).

The yardstick throughout: oracle.Spectrum(n) fed the channel IQ that wr_chan_fetch(WR_STAGE_CHAN_IQ) returns for that
receiver, frames [first_frame, first_frame + n); the comparison is speccases.check_db, unchanged (DB_ATOL
on bins within 60 dB of the row's peak).  The input carries noise at -50 dBFS so that every receiver's channel IQ is
non-zero, which is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import launch_plan
from speccases import check_db
from tunercases import bits_f32
from webradio_amd import capi, synth
from webradio_amd.device import Spectrum, Tuner

pytestmark = pytest.mark.gpu

FS, CHAN_RATE, AUDIO_RATE, D1, NRX = 2_400_000, 240_000, 48_000, 10, 70


def _rx_ifs(nrx=NRX):
    return [(c - nrx // 2) * 30_000 + 99 for c in range(nrx)]


def _stream(nframes, seed=1):
    return synth.fm_stream(nframes, FS, _rx_ifs()[3::16], amp=0.1, fm_base=700.0, fm_step=900.0, beta=2.0,
                           noise_dbfs=-50, seed=seed)


def _tuner(dev, max_block, nrx=NRX, max_channels=None, audio_rate=AUDIO_RATE, **rx):
    t = Tuner(dev, FS, max_channels or nrx, max_block, capi.WR_NCO_ROTATE)
    chans = [t.add_receiver(f, 100_000, CHAN_RATE, capi.WR_FM, 8_000, audio_rate, **rx) for f in _rx_ifs(nrx)]
    return t, chans


def _oracle_row(oracle, iq, first, n):
    o = oracle.Spectrum(n)
    o.process(np.ascontiguousarray(iq[2 * first: 2 * (first + n)], np.float32))
    assert o.frames_done == 1
    return o.get()


def _check_rows(oracle, t, chans, rows, first, n, k1, what):
    """rows[slot] against the oracle fed that receiver's fetched channel IQ"""
    for ch in chans:
        iq = t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1)
        assert iq.size == 2 * k1
        assert float(np.abs(iq[2 * first: 2 * (first + n)]).max()) > 0.0
        check_db(rows[t.slot(ch)], _oracle_row(oracle, iq, first, n), what)


# ---- sizes and offsets: 70 receivers (two lane groups, one ragged), ONE block of K1 = n + 16 channel frames ----------------

_cases = {}


@pytest.fixture(scope="module")
def sized(dev, oracle):
    """sized(n) -> (tuner, spectrum, k1, {channel: its fetched channel IQ}); built once per n, shared by the offsets"""
    def make(n):
        if n not in _cases:
            k1 = n + 16
            x = dev.upload(_stream(k1 * D1, seed=n))
            t, chans = _tuner(dev, k1 * D1)
            t.submit_device(x, k1 * D1)
            probe = chans if n <= 1024 else [ch for ch in chans if t.slot(ch) in (0, 63, 64, 69)]
            assert n <= 1024 or len(probe) == 4
            iqs = {ch: t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1) for ch in probe}
            dev.free(x)
            _cases[n] = (t, Spectrum(dev, n), k1, iqs)
        return _cases[n]
    yield make
    for t, spec, _, _ in _cases.values():
        spec.destroy()
        t.destroy()
    _cases.clear()


@pytest.mark.parametrize("where", ["0", "3", "end"])
@pytest.mark.parametrize("n", [8, 64, 1024, 8192])
def test_sizes_and_offsets(dev, oracle, sized, n, where):
    t, spec, k1, iqs = sized(n)
    first = {"0": 0, "3": 3, "end": k1 - n}[where]
    rows = t.chan_spectra(spec, first)
    assert rows.shape == (128, n)
    for ch, iq in iqs.items():
        assert iq.size == 2 * k1 and float(np.abs(iq[2 * first: 2 * (first + n)]).max()) > 0.0
        check_db(rows[t.slot(ch)], _oracle_row(oracle, iq, first, n), "slot %d first %d" % (t.slot(ch), first))
    assert spec.frames_done() == 0                       # the spectrum's own frame state is left alone


def test_a_single_receiver(dev, oracle):
    n, k1 = 512, 528
    x = dev.upload(_stream(k1 * D1, seed=2))
    t, chans = _tuner(dev, k1 * D1, nrx=1)
    spec = Spectrum(dev, n)
    t.submit_device(x, k1 * D1)
    rows = t.chan_spectra(spec, 5)
    assert rows.shape == (64, n)
    _check_rows(oracle, t, chans, rows, 5, n, k1, "single")
    spec.destroy()
    t.destroy()
    dev.free(x)


@pytest.mark.parametrize("nrx", [449, 961], ids=["512-slots", "1024-slots"])
def test_more_slots_than_compute_units(dev, oracle, nrx):
    """Columns share a workgroup only where there are more of them than compute units (wrp_fft_cols_ct; 256 on an MI355X: two
    columns per workgroup at 512 slots, four at 1024).  Rows at both ends of the first and of the last tile, and across a lane group."""
    n, k1 = 64, 80
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert launch_plan.fft_cols_ct(n, (nrx + 63) // 64 * 64, cus) > 1, "on this device the case does not reach the branch it is about"
    x = dev.upload(_stream(k1 * D1, seed=nrx))
    t = Tuner(dev, FS, nrx, k1 * D1, capi.WR_NCO_ROTATE)
    chans = [t.add_receiver((c % NRX - NRX // 2) * 30_000 + 99, 100_000, CHAN_RATE, capi.WR_FM, 8_000, AUDIO_RATE)
             for c in range(nrx)]
    spec = Spectrum(dev, n)
    t.submit_device(x, k1 * D1)
    rows = t.chan_spectra(spec, 11)
    slots = (nrx + 63) // 64 * 64
    assert rows.shape == (slots, n)
    want = {0, 1, 2, 3, 63, 64, 65, nrx - 4, nrx - 3, nrx - 2, nrx - 1}
    probe = [ch for ch in chans if t.slot(ch) in want]
    assert len(probe) == len(want)
    _check_rows(oracle, t, probe, rows, 11, n, k1, "%d slots" % slots)
    spec.destroy()
    t.destroy()
    dev.free(x)


# ---- the buffer that is read -------------------------------------------------------------------------------------------------

def test_after_a_streaming_launch(dev, oracle):
    """two blocks into a streaming launch, then the call: it closes the launch and reads the launch's own ring; the rows
    are the bits of the same blocks on a tuner that does not stream"""
    n, k1, first = 512, 640, 100
    x = dev.upload(_stream(2 * k1 * D1, seed=3))
    spec = Spectrum(dev, n)
    got = {}
    for stream in (False, True):
        t, chans = _tuner(dev, k1 * D1)
        t.streaming(stream)
        t.submit_device(x, k1 * D1)
        t.submit_device(x + 8 * k1 * D1, k1 * D1)
        assert t.stream_info()[0] is stream
        rows = t.chan_spectra(spec, first)
        assert t.stream_info()[0] is False
        if stream:
            assert t.stream_info()[2] == 2
        _check_rows(oracle, t, chans, rows, first, n, k1, "streaming" if stream else "per block")
        got[stream] = rows[[t.slot(ch) for ch in chans]]
        t.destroy()
    assert np.array_equal(bits_f32(got[True]), bits_f32(got[False]))
    spec.destroy()
    dev.free(x)


def test_with_a_second_channel_stage(dev, oracle):
    n, k1b = 64, 100                                     # 240 kHz -> 120 kHz: 100 frames at the demodulator's input
    nframes = 2 * k1b * D1
    x = dev.upload(_stream(nframes, seed=4))
    t, chans = _tuner(dev, nframes, audio_rate=24_000, stage2=(64, 50_000, 120_000))
    spec = Spectrum(dev, n)
    t.submit_device(x, nframes)
    rows = t.chan_spectra(spec, k1b - n)
    _check_rows(oracle, t, chans, rows, k1b - n, n, k1b, "second stage")
    spec.destroy()
    t.destroy()
    dev.free(x)


def test_with_a_128_tap_channel_filter(dev, oracle):
    n, k1 = 64, 100
    x = dev.upload(_stream(k1 * D1, seed=5))
    t, chans = _tuner(dev, k1 * D1, fir_lengths=(128, 64))
    spec = Spectrum(dev, n)
    t.submit_device(x, k1 * D1)
    rows = t.chan_spectra(spec, 7)
    _check_rows(oracle, t, chans, rows, 7, n, k1, "128 taps")
    spec.destroy()
    t.destroy()
    dev.free(x)


def test_with_a_held_block(dev, oracle):
    """wr_tuner_set_blocks_per_launch(2) and ONE block submitted: the call sends it out first"""
    n, k1 = 64, 100
    x = dev.upload(_stream(k1 * D1, seed=6))
    t, chans = _tuner(dev, 2 * k1 * D1)
    t.blocks_per_launch(2)
    spec = Spectrum(dev, n)
    t.submit_device(x, k1 * D1)
    rows = t.chan_spectra(spec, 36)
    _check_rows(oracle, t, chans, rows, 36, n, k1, "held block")
    spec.destroy()
    t.destroy()
    dev.free(x)


def test_db_dev_form_is_the_array_form(dev, oracle):
    n, k1 = 256, 272
    x = dev.upload(_stream(k1 * D1, seed=7))
    t, chans = _tuner(dev, k1 * D1)
    spec = Spectrum(dev, n)
    t.submit_device(x, k1 * D1)
    rows = t.chan_spectra(spec, 9)
    out = dev.malloc(128 * n * 4)
    assert t.chan_spectra(spec, 9, db_dev=out) == 128
    dev.sync()
    used = [t.slot(ch) for ch in chans]
    assert np.array_equal(bits_f32(dev.download(out, 128 * n).reshape(128, n)[used]), bits_f32(rows[used]))
    dev.free(out)
    spec.destroy()
    t.destroy()
    dev.free(x)


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _refused(dev, rc, status, word):
    assert rc == status
    assert word in dev.lib.wr_last_error()


def test_refusals(dev):
    from webradio_amd.device import Device
    lib = dev.lib
    k1 = 100
    x = dev.upload(_stream(k1 * D1, seed=8))
    out = dev.malloc(64 * 16384 * 4)
    o = C.c_void_p(out)
    t, chans = _tuner(dev, k1 * D1, nrx=2, max_channels=3)
    iq64, real64, big = Spectrum(dev, 64), Spectrum(dev, 64, real=True), Spectrum(dev, 16384)
    call = lib.wr_tuner_chan_spectra
    _refused(dev, call(t.h, iq64.h, 0, o, None), capi.WR_ERR_STATE, b"nothing submitted")
    t.submit_device(x, k1 * D1)
    _refused(dev, call(None, iq64.h, 0, o, None), capi.WR_ERR_ARG, b"NULL")
    _refused(dev, call(t.h, None, 0, o, None), capi.WR_ERR_ARG, b"NULL")
    _refused(dev, call(t.h, iq64.h, 0, None, None), capi.WR_ERR_ARG, b"NULL")
    _refused(dev, call(t.h, real64.h, 0, o, None), capi.WR_ERR_ARG, b"real")
    _refused(dev, call(t.h, big.h, 0, o, None), capi.WR_ERR_ARG, b"8192")
    _refused(dev, call(t.h, iq64.h, k1 - 63, o, None), capi.WR_ERR_ARG, b"beyond")
    _refused(dev, call(t.h, iq64.h, 2 ** 63, o, None), capi.WR_ERR_ARG, b"beyond")
    assert call(t.h, iq64.h, k1 - 64, o, None) == capi.WR_OK          # (the last frame that fits)
    other = Device(0)
    foreign = Spectrum(other, 64)
    _refused(dev, call(t.h, foreign.h, 0, o, None), capi.WR_ERR_ARG, b"another device")
    foreign.destroy()
    other.close()
    # a second rate group: one receiver at another channel rate
    t.add_receiver(5_000, 50_000, 120_000, capi.WR_FM, 8_000, 24_000)
    _refused(dev, call(t.h, iq64.h, 0, o, None), capi.WR_ERR_STATE, b"several rate groups")
    dev.sync()
    for s in (iq64, real64, big):
        s.destroy()
    t.destroy()
    dev.free(out)
    dev.free(x)
