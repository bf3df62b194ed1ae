"""-m gpu: the spectrum of REAL samples (wr_spectrum_create_real; the reference's FIXMEs at io/spectrumsink.cxx:62-64).

The definition: what the IQ sink gives for the frames (x[n], 0) -- so the oracle is oracle.Spectrum(n) fed (x, 0)
interleaved, and the tolerances are those of tests/speccases.py, unchanged: BIN_RTOL * the frame's peak bin on
all n complex bins, DB_ATOL on bins within 60 dB of the peak.  (A float32 emulation of this formulation -- radix-2
transform of n/2 packed points, untangle step, twiddles rounded from double -- stays within 1.2e-7 * peak of a float64
FFT for n = 8 ... 2^20: the bound has tenfold room.)  Every check prints the figures it then asserts on."""
import ctypes as C

import numpy as np
import pytest

from speccases import BIN_RTOL, check_db
from tunercases import bits_f32
from webradio_amd import capi, synth
from webradio_amd.device import Spectrum, Tuner

pytestmark = pytest.mark.gpu


def _real_stream(n, seed=1, fs=2_400_000):
    """the I part of an FM multiplex: three carriers and noise at -50 dBFS"""
    return np.ascontiguousarray(synth.fm_stream(n, fs, [100_000, -450_000, 700_001], amp=0.2, noise_dbfs=-50, seed=seed)[0::2])


def _with_zero_q(x):
    iq = np.zeros(2 * x.size, np.float32)
    iq[0::2] = x
    return iq


_want = {}


def _oracle_frame(oracle, x):
    """(dB row, bins) of the oracle's IQ sink fed (x, 0); computed once per distinct frame"""
    x = np.ascontiguousarray(x, np.float32)
    key = (x.size, hash(x.tobytes()))
    if key not in _want:
        o = oracle.Spectrum(x.size)
        o.process(_with_zero_q(x))
        assert o.frames_done == 1
        _want[key] = (o.get(), o.bins())
        if len(_want) > 64:
            _want.pop(next(iter(_want)))
    return _want[key]


def _check(spec, want, what=""):
    want_db, want_bins = want
    got_bins = spec.get_bins()
    peak = np.abs(want_bins[0::2] + 1j * want_bins[1::2]).max()
    err = float(np.abs(got_bins - want_bins).max())
    print("%s n=%d bin error %.3g x peak (bound %.3g)" % (what, want_db.size, err / peak, BIN_RTOL))
    assert err <= BIN_RTOL * peak
    check_db(spec.get_db(), want_db, what)


def _assert_symmetric(spec):
    n = spec.n
    z = spec.get_bins()
    re, im = z[0::2], z[1::2]
    k = np.arange(1, n // 2)
    assert np.array_equal(bits_f32(re[n - k]), bits_f32(re[k]))
    assert np.array_equal(bits_f32(im[n - k]), bits_f32(-im[k]))
    assert bits_f32(im[:1])[0] == 0 and bits_f32(im[n // 2: n // 2 + 1])[0] == 0      # exactly +0
    db = spec.get_db()
    j = np.arange(1, n // 2)
    assert np.array_equal(bits_f32(db[n // 2 + j]), bits_f32(db[n // 2 - j]))


# 8: a 4-point packed transform; 16384: the largest in one pass; 32768: the smallest with the untangle kernel;
# 131072: 65536 packed points; 1048576: the largest
@pytest.mark.parametrize("n", [8, 16, 512, 16384, 32768, 131072, 1048576])
def test_real_spectrum_sizes(dev, oracle, n):
    x = _real_stream(n, seed=n)
    s = Spectrum(dev, n, real=True)
    assert s.channels() == 1
    s.push_host(x)
    assert s.frames_done() == 1
    _check(s, _oracle_frame(oracle, x), "sizes")
    _assert_symmetric(s)
    s.destroy()


@pytest.mark.parametrize("n,b", [(8, 2), (512, 37), (16384, 4000), (32768, 5)])
def test_cosine_peaks_on_both_sides(dev, n, b):
    x = (0.5 * np.cos(2 * np.pi * b * np.arange(n) / n)).astype(np.float32)
    s = Spectrum(dev, n, real=True)
    s.push_host(x)
    db = s.get_db()
    top = sorted(int(i) for i in np.argsort(db)[-2:])
    assert top == [n // 2 - b, n // 2 + b]
    _assert_symmetric(s)
    s.destroy()


def test_frames_across_pushes_of_any_size(dev, oracle):
    """Frames straddle pushes of arbitrary -- odd -- sample counts (spectrumsink.cxx:101-121)."""
    n = 1024
    chunks = (100, 923, 1, 2047, 1501, 848)
    x = _real_stream(sum(chunks), seed=3)
    s, o = Spectrum(dev, n, real=True), oracle.Spectrum(n)
    with pytest.raises(capi.WrError):
        s.get_db()                                      # Q8: nothing transformed yet
    pos = 0
    for chunk in chunks:
        part = x[pos: pos + chunk]
        pos += chunk
        s.push_host(part)
        o.process(_with_zero_q(part))
        assert s.frames_done() == o.frames_done
        if o.frames_done:
            _check(s, (o.get(), o.bins()), "pushes")
    assert s.frames_done() == sum(chunks) // n
    s.destroy()


def _newest(x, pos, n, h):
    nfr = (pos - n) // h + 1 if pos >= n else 0
    return nfr, x[(nfr - 1) * h: (nfr - 1) * h + n]


ODD_HOPS = [(16, 5), (512, 333), (4096, 2048), (32768, 4097)]


@pytest.mark.parametrize("n,hop", ODD_HOPS)
def test_odd_hops_one_host_block(dev, oracle, n, hop):
    x = _real_stream(n + 6 * hop + 3, seed=hop)
    s = Spectrum(dev, n, hop, real=True)
    s.push_host(x)
    nfr, frame = _newest(x, x.size, n, hop)
    assert nfr == 7 and s.frames_done() == nfr
    _check(s, _oracle_frame(oracle, frame), "odd hop, host")
    _assert_symmetric(s)
    s.destroy()


@pytest.mark.parametrize("n,hop", ODD_HOPS)
def test_odd_hops_device_blocks(dev, oracle, n, hop):
    """WR_DEVICE blocks: the newest frame starts at an odd float offset of a device buffer (the in-place path), and what
    follows its hop is carried into the next push."""
    sizes = [n + hop + 1, n + 2 * hop + 2, 3, n + 3 * hop, n + hop, 2 * n + 5 * hop + 1]
    x = _real_stream(sum(sizes), seed=n + hop)
    s = Spectrum(dev, n, hop, real=True)
    pos, odd = 0, 0
    for sz in sizes:
        p = dev.upload(x[pos: pos + sz])
        s.push_device(p, sz)
        dev.sync()
        dev.free(p)
        nfr, frame = _newest(x, pos + sz, n, hop)
        odd += ((nfr - 1) * hop - pos) % 2 if (nfr - 1) * hop >= pos else 0
        pos += sz
        assert s.frames_done() == nfr
        _check(s, _oracle_frame(oracle, frame), "odd hop, device")
    if hop % 2:
        assert odd                                      # (an odd offset inside a block was among them)
    s.destroy()


@pytest.mark.parametrize("tail_only", [False, True], ids=["whole-block", "tail-only"])
@pytest.mark.parametrize("n,hop", [(1024, 0), (4096, 2048), (512, 0)])
def test_real_device_pushes_in_place(dev, oracle, n, hop, tail_only):
    """The size ladder of test_gpu_spectrum.test_device_pushes_in_place, in samples; tail-only: everything before the last
    n + hop samples of a block is NaN (nothing before the newest frame is read)."""
    h = hop or n
    sizes = [4 * n, 3 * n + 77, 5 * h - 77, 2 * n, n + 1, 6 * n, 2 * n + h + 5, 3 * n + 1]
    x = _real_stream(sum(sizes), seed=5)
    s = Spectrum(dev, n, hop, real=True)
    pos = 0
    for sz in sizes:
        part = np.array(x[pos: pos + sz])
        if tail_only and sz > n + h:
            part[: sz - (n + h)] = np.nan
        p = dev.upload(part)
        s.push_device(p, sz)
        dev.sync()
        dev.free(p)
        pos += sz
        nfr, frame = _newest(x, pos, n, h)
        assert s.frames_done() == nfr
        if nfr:
            _check(s, _oracle_frame(oracle, frame), "in place")
    s.destroy()


def _rows_dev(dev, spec, buf, stride, nrows, how="rows"):
    p = dev.upload(buf)
    out = dev.malloc(nrows * spec.n * 4)
    if how == "rows":
        spec.batch_db_rows(p, stride, nrows, out)
    else:
        spec.batch_db(p, nrows, out)
    dev.sync()
    got = dev.download(out, nrows * spec.n).reshape(nrows, spec.n)
    dev.free(p)
    dev.free(out)
    return got


@pytest.mark.parametrize("n,rows", [(64, 70), (32768, 5)])
@pytest.mark.parametrize("pad", [3, 0], ids=["stride-n+3", "stride-n"])
def test_batch_db_rows(dev, oracle, n, rows, pad):
    stride = n + pad
    x = _real_stream(rows * stride, seed=n + pad)
    s = Spectrum(dev, n, real=True)
    got = _rows_dev(dev, s, x, stride, rows)
    for r in range(rows):
        check_db(got[r], _oracle_frame(oracle, x[r * stride: r * stride + n])[0], "rows")
        j = np.arange(1, n // 2)
        assert np.array_equal(bits_f32(got[r][n // 2 + j]), bits_f32(got[r][n // 2 - j]))
    s.destroy()


@pytest.mark.parametrize("n,hop,frames", [(64, 21, 70), (32768, 4097, 5)])
def test_batch_db_reads_frames_a_hop_of_floats_apart(dev, oracle, n, hop, frames):
    x = _real_stream(n + (frames - 1) * hop, seed=hop)
    s = Spectrum(dev, n, hop, real=True)
    got = _rows_dev(dev, s, x, hop, frames, how="hop")
    for f in range(frames):
        check_db(got[f], _oracle_frame(oracle, x[f * hop: f * hop + n])[0], "batch_db")
    s.destroy()


@pytest.mark.parametrize("n,rows", [(512, 9), (16384, 3), (65536, 2)])
def test_rows_of_an_iq_spectrum_are_batch_db_s(dev, n, rows):
    """On an IQ spectrum wr_spectrum_batch_db_rows with row_stride = hop gives the bits of wr_spectrum_batch_db."""
    iq = synth.fm_stream(rows * n, 2_400_000, [250_000, -400_000], amp=0.3, seed=n)
    s = Spectrum(dev, n)
    assert s.channels() == 2
    a = _rows_dev(dev, s, iq, n, rows, how="hop")
    b = _rows_dev(dev, s, iq, n, rows, how="rows")
    assert np.array_equal(bits_f32(a), bits_f32(b))
    s.destroy()


def test_row_stride_below_the_frame_is_refused(dev):
    for real in (False, True):
        s = Spectrum(dev, 64, real=real)
        p = dev.malloc(4096)
        assert dev.lib.wr_spectrum_batch_db_rows(s.h, C.c_void_p(p), 63, 2, C.c_void_p(p)) == capi.WR_ERR_ARG
        assert b"row_stride" in dev.lib.wr_last_error()
        dev.free(p)
        s.destroy()


FS, CHAN_RATE, AUDIO_RATE, K2, NRX = 2_400_000, 240_000, 48_000, 128, 70


def _rx_ifs():
    return [(c - NRX // 2) * 30_000 + 99 for c in range(NRX)]


def _audio_tuner(dev, stream):
    t = Tuner(dev, FS, NRX, K2 * 50, capi.WR_NCO_ROTATE)
    chans = [t.add_receiver(f, 100_000, CHAN_RATE, capi.WR_FM, 8_000, AUDIO_RATE) for f in _rx_ifs()]
    t.streaming(stream)
    return t, chans


def _audio_rows(dev, t, spec):
    a, stride, frames = t.audio_dev()
    assert frames == K2 and stride >= K2
    slots = t.fetch_audio_all().shape[0]
    out = dev.malloc(slots * spec.n * 4)
    spec.batch_db_rows(a, stride, slots, out)
    dev.sync()
    rows = dev.download(out, slots * spec.n).reshape(slots, spec.n)
    dev.free(out)
    return rows


def test_audio_spectra_of_every_receiver_of_a_tuner(dev, oracle):
    """70 receivers (two lane groups, one ragged), one block of 128 audio frames: wr_spectrum_batch_db_rows on
    wr_tuner_audio_dev's rows, row by row against the oracle fed that receiver's fetched audio as (x, 0).  A tuner that
    does not stream keeps stream_info() as it was; the call closes the launch of one that does, and the rows are the same."""
    n = K2
    iq = synth.fm_stream(2 * K2 * 50, FS, _rx_ifs()[3::16], amp=0.1, fm_base=700.0, fm_step=900.0, beta=2.0)
    x = dev.upload(iq)
    spec = Spectrum(dev, n, real=True)

    t, chans = _audio_tuner(dev, False)
    t.submit_device(x, K2 * 50)
    before = t.stream_info()
    rows = _audio_rows(dev, t, spec)
    assert t.stream_info() == before and before[0] is False
    for ch in chans:
        audio = t.fetch(ch, capi.WR_STAGE_AUDIO, K2)
        assert audio.size == K2
        if float(np.abs(audio).max()) > 0.0:
            check_db(rows[t.slot(ch)], _oracle_frame(oracle, audio)[0], "tuner")
    assert any(float(np.abs(t.fetch(ch, capi.WR_STAGE_AUDIO, K2)).max()) > 0.0 for ch in chans)
    t.submit_device(x + 8 * K2 * 50, K2 * 50)
    rows2 = _audio_rows(dev, t, spec)
    t.destroy()

    t, chans = _audio_tuner(dev, True)
    t.submit_device(x, K2 * 50)
    assert t.stream_info()[0] is True
    a, stride, frames = t.audio_dev()                   # (reading the audio closes the launch ...)
    t.submit_device(x + 8 * K2 * 50, K2 * 50)           # (... and the next block opens another)
    assert t.stream_info()[0] is True
    out = dev.malloc(spec.n * 4)
    spec.batch_db_rows(a, stride, 1, out)               # a call on the device while the launch is open: closes it first
    assert t.stream_info()[0] is False
    dev.sync()
    dev.free(out)
    srows2 = _audio_rows(dev, t, spec)
    used = [t.slot(ch) for ch in chans]
    assert np.array_equal(bits_f32(srows2[used]), bits_f32(rows2[used]))
    t.destroy()
    spec.destroy()
    dev.free(x)


@pytest.mark.parametrize("n", [512, 32768])
def test_iq_spectrum_of_the_same_samples_is_unchanged(dev, oracle, n):
    """The same samples with zeros for Q through an ordinary Spectrum: the same oracle values, the same tolerances."""
    x = _real_stream(n, seed=n)
    s = Spectrum(dev, n)
    s.push_host(_with_zero_q(x))
    _check(s, _oracle_frame(oracle, x), "IQ with zeros")
    s.destroy()
