"""-m gpu: every bin of every transform size and batch path of the SpectrumSink (wr_fft.hip, wr_spectrum.hip).

The other spectrum modules feed synth.fm_stream -- a few carriers over noise 50 to 60 dB below them -- and compare dB on
bins within 60 dB of the frame's peak: that is 0.1 ... 70 % of the bins, and the batch entry points, which put out dB
only, are held on nothing else.  Here the input is flat (tests/flat_spectrum.py), the same mask keeps all but a handful
of bins -- asserted on every frame: at most MASK_OUT_SHARE of them are left out -- and every row of every batch is looked
at.  The reference is oracle.spectrum_np (float32 window and product, float64 FFT), which
tests/test_spectrum_flat_reference.py holds to oracle.Spectrum.

Tolerances: BIN_RTOL and DB_ATOL of tests/speccases.py, unchanged.  A float32 radix-2 Stockham restatement of
one frame of this input in numpy stays within 1.9e-7 * peak and 4e-4 dB up to 2^20 points: tenfold room.
Every check prints the figures it then asserts on (the lines that start with "all-bins:")."""
import numpy as np
import pytest

import wr_oracle
from flat_spectrum import MASK_OUT_SHARE, bin_error, db_error, flat, frames_of, interleaved, rows_db_error
from speccases import BIN_RTOL, DB_ATOL
from webradio_amd.device import Spectrum

pytestmark = pytest.mark.gpu


def _say(what, n, **figures):
    print("all-bins: %-34s n=%-8d %s" % (what, n, "  ".join(("%s=%d" if isinstance(v, int) else "%s=%.3g") % (k, v)
                                                            for k, v in figures.items())))


def _check_newest(spec, frame, what):
    """get_bins and get_db of `spec` against the reference of `frame` (complex64), all bins"""
    n = frame.size
    want_db, want_bins = wr_oracle.spectrum_np(np.ascontiguousarray(frame))
    berr = bin_error(spec.get_bins(), want_bins)
    derr, out = db_error(spec.get_db(), want_db)
    _say(what, n, bins_x_peak=berr, dB=derr, left_out=out)
    assert out <= MASK_OUT_SHARE * n
    assert berr <= BIN_RTOL
    assert derr <= DB_ATOL


def _batch(dev, spec, stream, rows, how="hop", stride=0):
    p = dev.upload(stream)
    out = dev.malloc(rows * spec.n * 4)
    if how == "rows":
        spec.batch_db_rows(p, stride, rows, out)
    else:
        spec.batch_db(p, rows, out)
    dev.sync()
    got = dev.download(out, rows * spec.n).reshape(rows, spec.n)
    dev.free(p)
    dev.free(out)
    return got


def _check_rows(got, stream, n, hop, frames, what, real=False):
    derr, out = rows_db_error(got, stream, n, hop, frames, real)
    _say(what, n, hop=hop, frames=frames, dB=derr, left_out=out)
    assert out <= MASK_OUT_SHARE * n
    assert derr <= DB_ATOL


# ---- every IQ size: k_fft_single to 8192, the generic four-step square (16384, 262144, 1048576) and not (32768, 131072,
# 524288: lds_fft's table sampled `scale` times finer), the 65536-point register path; k_bins_to_db strides from 524288 on
@pytest.mark.parametrize("n", [1 << b for b in range(3, 21)])
def test_every_iq_size(dev, oracle, n):
    iq = flat(2 * n, seed=100 + n)
    s = Spectrum(dev, n)
    s.push_host(iq)
    assert s.frames_done() == 1
    _check_newest(s, iq.view(np.complex64), "one frame pushed")
    s.destroy()


def test_small_plan_then_large_plan(dev, oracle):
    """The limit on a kernel's dynamic LDS is raised once per device and kernel and then remembered.  So, in one test on
    one device, every such kernel first at a size that needs no raised limit and then at its largest LDS: the one order
    in which a remembered limit could be too small."""
    for real, small, large in [(False, 8, 8192),            # k_fft_single: 128 B, then 128 KiB
                               (False, 16384, 262144),      # k_fft_pass1<false> and k_fft_pass2: 32 KiB, then 128 KiB
                               (True, 16, 16384),           # k_fft_real_single
                               (True, 32768, 524288)]:      # k_fft_pass1<true>, and k_fft_pass2 again, from a real plan
        for n in (small, large):
            x = flat(n if real else 2 * n, seed=900 + n)
            s = Spectrum(dev, n, real=real)
            s.push_host(x)
            assert s.frames_done() == 1
            _check_newest(s, x if real else x.view(np.complex64), "small then large, %s" % ("real" if real else "IQ"))
            s.destroy()


BATCHES = [
    # k_fft_single
    (8, 3, 300), (512, 128, 70), (8192, 1000, 9),
    # the generic four-step (blockIdx.y = frame), square and not; the last over its chunk of 128 MB = 16 frames by one
    (16384, 4096, 7), (32768, 5000, 5), (131072, 16384, 3), (1048576, 65536, 2), (1048576, 4096, 17),
    # 65536 points, one frame per pass-1 workgroup
    (65536, 32768, 5), (65536, 1000, 5),
    # four frames per workgroup: the rows a frame shares with the next kept in registers (24 groups and one of two frames),
    # any other hop (a last group of one), and over the chunk of 256 frames (then 3 frames, one per workgroup)
    (65536, 32768, 98), (65536, 4096, 97), (65536, 1024, 259),
]


@pytest.mark.parametrize("n,hop,frames", BATCHES, ids=["%d-%d-%d" % b for b in BATCHES])
def test_batch_db_every_row_every_bin(dev, oracle, n, hop, frames):
    iq = flat(2 * (n + (frames - 1) * hop), seed=n + hop + frames)
    s = Spectrum(dev, n, hop)
    got = _batch(dev, s, iq, frames)
    s.destroy()
    _check_rows(got, iq, n, hop, frames, "batch_db")


@pytest.mark.parametrize("n,hop", [(65536, 32768), (32768, 5000)])
def test_one_spectrum_through_a_life(dev, oracle, n, hop):
    """The work area between the passes holds one frame after create, is used by a push, grown by a batch of 5 and again
    by one of 100 frames, and then used by a push again."""
    stream = flat(2 * (n + 99 * hop), seed=7 * n)
    pushed = flat(2 * 2 * n, seed=7 * n + 1)
    s = Spectrum(dev, n, hop)
    s.push_host(pushed[: 2 * n])
    assert s.frames_done() == 1
    _check_newest(s, pushed[: 2 * n].view(np.complex64), "life: first push")
    for frames in (5, 100):
        got = _batch(dev, s, stream, frames)
        _check_rows(got, stream, n, hop, frames, "life: batch_db")
    s.push_host(pushed[2 * n:])
    nfr = (2 * n - n) // hop + 1
    assert s.frames_done() == nfr
    _check_newest(s, frames_of(pushed, n, hop)[nfr - 1], "life: push after the batches")
    s.destroy()


@pytest.mark.parametrize("n,hop", [(65536, 32768), (32768, 8192)])
def test_device_pushes_in_place_on_the_two_pass_sizes(dev, oracle, n, hop):
    """Blocks in device memory whose newest frame is transformed where it lies (test_gpu_spectrum.
    test_device_pushes_in_place, tail-only: everything in front of the last n + hop frames of a block is NaN), on the
    register path and the generic four-step."""
    sizes = [4 * n, 3 * n + 77, n + 1, 2 * n + hop + 5]
    iq = flat(2 * sum(sizes), seed=n + hop)
    s = Spectrum(dev, n, hop)
    pos = 0
    for sz in sizes:
        part = np.array(iq[2 * pos: 2 * (pos + sz)])
        if sz > n + hop:
            part[: 2 * (sz - (n + hop))] = np.nan
        p = dev.upload(part)
        s.push_device(p, sz)
        dev.sync()
        dev.free(p)
        pos += sz
        nfr = (pos - n) // hop + 1
        assert s.frames_done() == nfr
        _check_newest(s, frames_of(iq[: 2 * pos], n, hop)[nfr - 1], "device block of %d" % sz)
    s.destroy()


PALETTE_MID_DB = -37.0          # the palette runs from -50 to -25 dB (waterfall.js:94-106)


@pytest.mark.parametrize("n", [512, 65536, 1 << 20])
def test_waterfall_rows_on_all_columns(dev, oracle, n):
    """k_waterfall_row against oracle.waterfall_row on the reference's bins: dB on ALL columns, the palette by the rule of
    test_waterfall_row_for_the_ui.  The noise is scaled so that the row's median column lies near the palette's middle --
    by a power of two, which scales the reference's bins exactly; per row shape, because peak hold over n / width bins
    lifts a column by up to 11 dB -- and at least half of the reference's palette values must lie inside the palette, or
    the palette check would be vacuous."""
    iq = flat(2 * n, seed=3 * n)
    _, bins = wr_oracle.spectrum_np(iq.view(np.complex64))
    unit = interleaved(bins)
    s = Spectrum(dev, n)
    for width in sorted({n, n // 2, 512, 8, 1}, reverse=True):
        for hold in (0, 1):
            med = float(np.median(oracle.waterfall_row(unit, width, hold)[0]))
            gain = 2.0 ** round((PALETTE_MID_DB - med) / (20.0 * np.log10(2.0)))
            s.push_host(iq * np.float32(gain))
            wdb, wpal = oracle.waterfall_row(unit * gain, width, hold)
            gdb, gpal = s.waterfall_row(width, hold)
            inside = float(((wpal > 0) & (wpal < 255)).mean())
            err = float(np.abs(gdb.astype(np.float64) - wdb).max())
            step = int(np.abs(gpal.astype(int) - wpal.astype(int)).max())
            same = float((gpal == wpal).mean())
            _say("waterfall width %d hold %d" % (width, hold), n, median_dB=float(np.median(wdb)), inside_palette=inside,
                 dB=err, palette_step=step, palette_equal=same)
            assert abs(float(np.median(wdb)) - PALETTE_MID_DB) <= 3.1
            assert inside >= 0.5
            assert err <= DB_ATOL
            assert step <= 1
            assert same > 0.9
    s.destroy()


REAL_BATCHES = [(65536, 1001, 6),           # 256 x 128 packed points
                (1048576, 4097, 17)]        # 1024 x 512, over its chunk of 16 frames by one


@pytest.mark.parametrize("how", ["batch_db", "rows"])
@pytest.mark.parametrize("n,hop,frames", REAL_BATCHES, ids=["%d-%d-%d" % b for b in REAL_BATCHES])
def test_real_batches_every_row_every_bin(dev, oracle, n, hop, frames, how):
    """Real samples, flat: every dB value of every row against the definition, the IQ sink fed (x, 0).  Hops in floats, odd:
    every other frame starts off an 8-byte boundary.  wr_spectrum_batch_db_rows refuses a stride below the frame, so its
    rows lie n + hop apart."""
    stride = hop if how == "batch_db" else n + hop
    x = flat(n + (frames - 1) * stride, seed=n + stride)
    s = Spectrum(dev, n, hop, real=True)
    got = _batch(dev, s, x, frames, "rows" if how == "rows" else "hop", stride)
    s.destroy()
    _check_rows(got, x, n, stride, frames, "real " + how, real=True)
