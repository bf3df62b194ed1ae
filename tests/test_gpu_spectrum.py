"""-m gpu: SpectrumSink (wr_spectrum_*) against the oracle.

Tolerance (tests/speccases.py): complex bins agree within BIN_RTOL * max|X|; dB values are compared
on bins within 60 dB of the frame's peak with DB_ATOL."""
import numpy as np
import pytest

from speccases import BIN_RTOL, DB_ATOL, db_error
from webradio_amd import capi, synth
from webradio_amd.device import Spectrum

pytestmark = pytest.mark.gpu


def _check(spec_db, spec_bins, want_db, want_bins):
    peak = np.abs(want_bins[0::2] + 1j * want_bins[1::2]).max()
    assert np.abs(spec_bins - want_bins).max() <= BIN_RTOL * peak
    assert db_error(spec_db, want_db) <= DB_ATOL


@pytest.mark.parametrize("n", [8, 512, 4096, 8192, 16384, 65536])
def test_spectrum_sizes(dev, oracle, n):
    fs = 2_400_000
    iq = synth.fm_stream(n, fs, [100_000, -450_000, 700_001], amp=0.2, noise_dbfs=-50, seed=n)
    s = Spectrum(dev, n)
    s.push_host(iq)
    assert s.frames_done() == 1
    o = oracle.Spectrum(n)
    o.process(iq)
    _check(s.get_db(), s.get_bins(), o.get(), o.bins())
    s.destroy()


def test_default_size_known_answer(dev):
    # N = 512, tone at +100 kHz, fs 2.4 M -> peak bin 277
    n = 512
    t = np.arange(n) / 2_400_000.0
    z = 0.5 * np.exp(2j * np.pi * 100_000 * t)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    s = Spectrum(dev, n)
    s.push_host(iq)
    assert int(np.argmax(s.get_db())) == 277
    s.destroy()


def test_streaming_partial_frames(dev, oracle):
    """Frames straddle pushes of arbitrary size (spectrumsink.cxx:101-121)."""
    n = 1024
    iq = synth.fm_stream(5 * n + 300, 2_400_000, [250_000], amp=0.3)
    s, o = Spectrum(dev, n), oracle.Spectrum(n)
    with pytest.raises(capi.WrError):
        s.get_db()                                      # Q8: nothing transformed yet
    pos = 0
    for chunk in (100, 924, 1, 2047, 1500, 848):
        part = iq[2 * pos: 2 * (pos + chunk)]
        pos += chunk
        s.push_host(part)
        o.process(part)
        assert s.frames_done() == o.frames_done
        if o.frames_done:
            _check(s.get_db(), s.get_bins(), o.get(), o.bins())
    s.destroy()


@pytest.mark.parametrize("tail_only", [False, True], ids=["whole-block", "tail-only"])
@pytest.mark.parametrize("n,hop", [(1024, 0), (4096, 2048), (512, 0)])
def test_device_pushes_in_place(dev, oracle, n, hop, tail_only):
    """Blocks that already lie in device memory (the staged tuner block): with nothing carried over the most
    recent frame is transformed where it lies and only the tail is kept (r03); blocks that are not a
    multiple of the hop leave a tail, the next push takes the staged path and carries it on.  Against the
    oracle fed the same stream (spectrumsink.cxx:101-121), push after push."""
    h = hop or n
    sizes = [4 * n, 3 * n + 77, 5 * h - 77, 2 * n, n + 1, 6 * n, 2 * n + h + 5, 3 * n + 1]   # exact, ragged, back to exact, ...
    iq = synth.fm_stream(sum(sizes), 2_400_000, [250_000, -400_000], amp=0.3)
    s = Spectrum(dev, n, hop)
    pos, done = 0, 0
    for sz in sizes:
        part = np.array(iq[2 * pos: 2 * (pos + sz)])
        if tail_only and sz > n + h:
            # r04: a block of fftSize + hop frames or more is read from its most recent complete frame on, whatever was
            # carried over: the host runtime stages only that tail of a source block (stagedTail) -- the rest is NaN here
            part[: 2 * (sz - (n + h))] = np.nan
        p = dev.upload(part)
        s.push_device(p, sz)
        dev.sync()
        dev.free(p)
        pos += sz
        nfr = (pos - n) // h + 1 if pos >= n else 0                            # frames complete so far
        assert s.frames_done() == nfr
        if nfr:
            o = oracle.Spectrum(n)
            o.process(iq[2 * (nfr - 1) * h: 2 * ((nfr - 1) * h + n)])          # the most recent frame's samples
            _check(s.get_db(), s.get_bins(), o.get(), o.bins())
    s.destroy()


def test_overlap_hop(dev, oracle):
    """50 % overlap (BASELINE config 3): each frame is an ordinary reference frame fed the
    overlapped samples explicitly."""
    n, hop = 4096, 2048
    iq = synth.fm_stream(n + 5 * hop, 2_400_000, [-300_000], amp=0.3)
    s = Spectrum(dev, n, hop)
    s.push_host(iq)
    assert s.frames_done() == 6
    o = oracle.Spectrum(n)
    o.process(iq[2 * 5 * hop: 2 * (5 * hop + n)])
    _check(s.get_db(), s.get_bins(), o.get(), o.bins())
    s.destroy()


def test_batch_waterfall_rows(dev, oracle):
    import torch
    n, hop, rows = 65536, 32768, 5
    iq = synth.fm_stream(n + (rows - 1) * hop, 100_000_000, [12_500_000, -30_000_000], amp=0.3)
    x = torch.from_numpy(iq).cuda()
    out = torch.empty(rows * n, dtype=torch.float32, device="cuda")
    s = Spectrum(dev, n, hop)
    s.batch_db(x, rows, out)
    dev.sync()
    got = out.cpu().numpy().reshape(rows, n)
    for r in (0, 3, 4):
        frame = iq[2 * r * hop: 2 * (r * hop + n)]
        o = oracle.Spectrum(n)
        o.process(frame)
        want = o.get()
        strong = want >= want.max() - 60.0
        assert np.abs(got[r][strong] - want[strong]).max() <= DB_ATOL
    s.destroy()


def test_bad_sizes(dev):
    import ctypes as C
    h = C.c_void_p()
    assert dev.lib.wr_spectrum_create(C.byref(h), dev.h, 500, 0) == capi.WR_ERR_ARG   # spectrumsink.cxx:53-56
    assert b"power of 2" in dev.lib.wr_last_error()
    assert dev.lib.wr_spectrum_create(C.byref(h), dev.h, 512, 1024) == capi.WR_ERR_ARG


def test_waterfall_row_for_the_ui(dev, oracle):
    """the row the browser draws (dB, fft-shift, column reduction, palette index)
    produced on the device.  dB within DB_ATOL on strong columns; palette index equal except
    where the dB difference straddles a palette step (at most one step)."""
    n, width = 65536, 512
    iq = synth.fm_stream(n, 100_000_000, [12_500_000, -30_000_000, 3_000], amp=0.2, noise_dbfs=-60)
    s = Spectrum(dev, n)
    s.push_host(iq)
    o = oracle.Spectrum(n)
    o.process(iq)
    for hold in (0, 1):
        gdb, gpal = s.waterfall_row(width, hold)
        wdb, wpal = oracle.waterfall_row(o.bins(), width, hold)
        strong = wdb >= wdb.max() - 60.0
        assert np.abs(gdb - wdb)[strong].max() <= DB_ATOL
        assert np.abs(gpal.astype(int) - wpal.astype(int)).max() <= 1
        assert (gpal == wpal).mean() > 0.9
    # peak hold keeps narrow carriers that plain overdraw can lose
    assert s.waterfall_row(width, 1)[0].max() >= s.waterfall_row(width, 0)[0].max()
    with pytest.raises(capi.WrError):
        s.waterfall_row(500)
    s.destroy()
    # an all-zero frame: log10f(0) = -inf -> -10000 -> palette 0 (waterfallhandler.cxx:65-68)
    z = Spectrum(dev, 512)
    z.push_host(np.zeros(1024, np.float32))
    db, pal = z.waterfall_row(512)
    assert (db == -10000.0).all() and (pal == 0).all()
    z.destroy()


@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("WR_FUZZ_SEEDS", "10"))))
def test_random_device_pushes_with_only_the_tail_staged(dev, oracle, seed):
    """Seeded fuzz of wr_spectrum_push(WR_DEVICE): random frame sizes, hops and push lengths (shorter than a frame, ragged,
    many frames long); of every push of fftSize + hop frames or more only the last fftSize + hop frames are real, the rest
    NaN -- what the host runtime's stagedTail hands the SpectrumSink.  Frame count and the most recent frame against the
    oracle fed the whole stream, push after push."""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([64, 256, 1024, 4096]))
    h = int(rng.choice([n, n // 2, n // 4, 3 * n // 4]))
    sizes = [int(rng.choice([1, n // 3 + 1, n - 1, n, n + h - 1, n + h, 2 * n + 5, 7 * h + 3, 12 * n + int(rng.integers(0, n))]))
             for _ in range(8)]
    iq = synth.fm_stream(sum(sizes), 2_400_000, [250_000, -400_000], amp=0.3, seed=seed)
    s = Spectrum(dev, n, h)
    pos = 0
    for sz in sizes:
        part = np.array(iq[2 * pos: 2 * (pos + sz)])
        if sz >= n + h:
            part[: 2 * (sz - (n + h))] = np.nan
        p = dev.upload(part)
        s.push_device(p, sz)
        dev.sync()
        dev.free(p)
        pos += sz
        nfr = (pos - n) // h + 1 if pos >= n else 0
        assert s.frames_done() == nfr, (n, h, sizes)
        if nfr:
            o = oracle.Spectrum(n)
            o.process(iq[2 * (nfr - 1) * h: 2 * ((nfr - 1) * h + n)])
            _check(s.get_db(), s.get_bins(), o.get(), o.bins())
    s.destroy()
