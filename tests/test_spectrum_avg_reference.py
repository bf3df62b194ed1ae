"""wr_spectrum_batch_avg without a GPU: the reference of tests/test_gpu_spectrum_avg.py alone keeps that module's mask
honest, the float32 restatement of the rule agrees with it, the burst has its known answer, and the plan of a call
(webradio_amd/csrc/wr_plan.h: chunks, scratch cap, launch count) keeps its promises."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import launch_plan
import specavg_np as sa
import wr_oracle as oracle
from flat_spectrum import MASK_OUT_SHARE, flat, interleaved
from speccases import DB_ATOL
from webradio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ([(False,) + s + (1, 0) for s in sa.IQ_SHAPES] + [(True,) + s + (1, 0) for s in sa.REAL_SHAPES] + sa.GROUP_SHAPES)


NEW = ("wr_spectrum_batch_avg", "wr_spectrum_rows_waterfall")


@pytest.fixture(autouse=True)
def _the_calls_exist():
    """this module's references and plan are those of the two calls: without them in the library and the binding nothing
    here means anything"""
    lib = capi.load()
    for name in NEW:
        assert name in capi.SIGNATURES and hasattr(lib, name), name


def test_the_abi_version_stays():
    assert capi.load().wr_abi_version() == capi.WR_ABI_VERSION == 6


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()
    assert lib.wr_spectrum_batch_avg(None, None, 1, 1, 0, 0, None, None) == capi.WR_ERR_ARG
    assert b"wr_spectrum_batch_avg" in lib.wr_last_error()
    assert lib.wr_spectrum_rows_waterfall(None, None, 1, 8, 0, None, None) == capi.WR_ERR_ARG
    assert b"wr_spectrum_rows_waterfall" in lib.wr_last_error()


@pytest.mark.parametrize("shape", SHAPES, ids=["%s-%d-%d-%d-%d-%d" % (("real" if s[0] else "iq",) + s[1:]) for s in SHAPES])
def test_mask_keeps_nearly_every_bin_of_the_mean_and_peak_rows(shape):
    """With the reference alone, on the flat input and seeds the GPU module uses: of every mean and peak row at most
    MASK_OUT_SHARE of the bins lie more than MASK_DB below the row's peak."""
    n = shape[1]
    _, mean, peak = sa.reference_of(*shape)
    for what, rows in (("mean", mean), ("peak", peak)):
        out = int((rows < rows.max(axis=-1, keepdims=True) - sa.MASK_DB).sum(axis=-1).max())
        print("avg-reference: %s n=%d %s rows: the mask leaves out %d bins at most" % ("real" if shape[0] else "IQ", n, what, out))
        assert out <= MASK_OUT_SHARE * n


@pytest.mark.parametrize("n,hop", [(512, 128), (65536, 1024)])
def test_restatement_agrees_with_the_reference(n, hop):
    """The float32 restatement on float64 bins rounded to float32, F = 259, against the float64 reference: within a tenth
    of DB_ATOL on the masked bins.  The figure printed is the room the order of summation (and the rounding of the bins
    to float32) leaves: the GPU test holds the device to DB_ATOL."""
    F = 259
    frames = sa.group_frames(flat(2 * sa.span(n, hop, F), seed=n + F), False, n, hop, F)
    bins32 = interleaved(oracle.spectrum_np(frames)[1]).astype(np.float32)
    mean, peak = sa.restate_linear(bins32)
    want_mean, want_peak = sa.reference_db(frames)
    e_mean, _ = sa.masked_error(sa.to_db64(mean, n), want_mean)
    e_peak, _ = sa.masked_error(sa.to_db64(peak, n), want_peak)
    print("avg-reference: restatement against reference n=%d F=%d: mean %.3g dB, peak %.3g dB (bound %.3g)"
          % (n, F, e_mean, e_peak, DB_ATOL / 10))
    assert e_mean <= DB_ATOL / 10 and e_peak <= DB_ATOL / 10


def test_restatement_of_one_frame_is_that_frame():
    bins = interleaved(oracle.spectrum_np(flat(2 * 64, seed=1).view(np.complex64))[1]).astype(np.float32)[None]
    mean, peak = sa.restate_linear(bins)
    assert np.array_equal(mean.view(np.uint32), peak.view(np.uint32))
    assert np.array_equal(peak, np.fft.fftshift(sa.power32(bins)[0]))


def test_burst_known_answer_on_the_reference():
    """Eight frames of 512 points, a carrier on a bin centre in frame 3 only, noise 50 dB below it everywhere: at the
    carrier's bin the peak row is frame 3's row, the mean row lies 10*log10(8) below it, the last frame's row does not
    show it."""
    n, F = sa.BURST_N, sa.BURST_F
    frames = sa.group_frames(sa.burst_stream(), False, n, n, F)
    rows = oracle.spectrum_np(frames)[0]
    mean, peak = sa.reference_db(frames)
    col = sa.BURST_COLUMN
    assert int(np.argmax(rows[sa.BURST_AT])) == col
    print("avg-reference: burst: frame 3 %.3f dB, peak %.3f, mean %.3f, frame 7 %.3f"
          % (rows[sa.BURST_AT, col], peak[col], mean[col], rows[F - 1, col]))
    assert abs(peak[col] - rows[sa.BURST_AT, col]) <= 1e-9
    assert abs((peak[col] - mean[col]) - 10.0 * np.log10(8.0)) <= 0.05
    assert rows[F - 1, col] < peak[col] - 40.0


def test_rows_waterfall_restatement_is_the_oracle_s():
    """the restatement for rows against oracle.waterfall_row (bins in, dB inside), on the dB the oracle itself makes"""
    n = 512
    iq = flat(2 * n, seed=9) * np.float32(1.0 / 64)
    o = oracle.Spectrum(n)
    o.process(iq)
    for width in (n, n // 2, 8, 1):
        for hold in (0, 1):
            wdb, wpal = oracle.waterfall_row(o.bins(), width, hold)
            gdb, gpal = sa.rows_waterfall(o.get(), width, hold)
            assert np.array_equal(gdb[0], wdb) and np.array_equal(gpal[0], wpal)
    db, pal = sa.rows_waterfall(np.full(16, -np.inf, np.float32), 4, 1)
    assert np.all(db == -10000.0) and np.all(pal == 0)


# ---- the plan ---------------------------------------------------------------------------------------------------------------

SIZE = C.c_size_t
WR_FFT_SINGLE = 0
NS, FS, GS = (8, 8192, 65536, 1048576), (1, 259, 100_000), (1, 256, 65_535)


@pytest.fixture(scope="module")
def plan():
    return launch_plan.lib()


def _plan(lib, n, F, G):
    out = (SIZE * 4)()
    lib.spec_avg_plan(n, F, G, out)
    return tuple(out)


def _chunks(lib, n, F, G, most):
    rows = (SIZE * (4 * most))()
    count = lib.spec_avg_chunks(n, F, G, most, rows)
    assert count <= most, "more chunks than the test walks"
    return np.array(rows[: 4 * count], dtype=np.int64).reshape(count, 4)


def test_the_cap_is_of_the_work_area_s_order(plan):
    """FFT_WORK_BYTES is 128 MB"""
    assert 32 << 20 <= plan.spec_avg_cap_bytes() <= 128 << 20


@pytest.mark.parametrize("n,F,G", list(itertools.product(NS, FS, GS)))
def test_chunks_stay_within_the_scratch_cap(plan, n, F, G):
    """bins of a chunk (8 n bytes a frame) and the carry (8 n bytes a group, where a group's frames are cut) fit the cap;
    a chunk is never empty; the reduce grid gives every (group, bin) of a chunk a thread"""
    cap = plan.spec_avg_cap_bytes()
    fchunk, gchunk, carry, nbytes = _plan(plan, n, F, G)
    assert 1 <= fchunk <= F and 1 <= gchunk <= G
    assert nbytes == (fchunk * gchunk + carry) * n * 8 <= cap
    assert carry == (gchunk if fchunk < F else 0)
    assert gchunk == 1 or fchunk == F                       # several groups share a chunk only whole
    assert plan.spec_avg_reduce_grid(n, gchunk) * 256 >= gchunk * n > (plan.spec_avg_reduce_grid(n, gchunk) - 1) * 256
    assert gchunk * fchunk < 2 ** 31                        # one launch's frames: grid.x


@pytest.mark.parametrize("n,F,G", [(n, F, G) for n, F, G in itertools.product(NS, FS, GS)
                                   if -(-F * G * n * 8 // (32 << 20)) <= 200_000])
def test_chunks_cover_every_frame_once_in_order(plan, n, F, G):
    """Groups ascend; within a group the frames ascend without gap or overlap from 0 to F; every group is there once.
    (The combinations with more than some 200 000 chunks are left to the closed form below.)"""
    fchunk, gchunk, _, _ = _plan(plan, n, F, G)
    ch = _chunks(plan, n, F, G, 450_000)
    g0, ng, f0, nf = ch.T
    assert np.all(ng >= 1) and np.all(nf >= 1) and np.all(ng <= gchunk) and np.all(nf <= fchunk)
    starts = f0 == 0
    assert starts[0] and g0[0] == 0
    # a chunk either continues its groups' frames or begins the next groups
    cont = ~starts[1:]
    assert np.all(g0[1:][cont] == g0[:-1][cont]) and np.all(ng[1:][cont] == ng[:-1][cont])
    assert np.all(f0[1:][cont] == (f0 + nf)[:-1][cont])
    nxt = starts[1:]
    assert np.all((f0 + nf)[:-1][nxt] == F) and np.all(g0[1:][nxt] == (g0 + ng)[:-1][nxt])
    assert f0[-1] + nf[-1] == F and g0[-1] + ng[-1] == G
    assert int((ng * nf).sum()) == F * G


def test_chunks_of_a_small_case_by_hand(plan):
    """n = 1048576: 8 frames fit 64 MB.  F = 17 > 8: chunks of 7 frames and the carry; two groups, one after the other."""
    if plan.spec_avg_cap_bytes() != 64 << 20:
        pytest.fail("the hand-worked case is for a cap of 64 MB")
    assert _plan(plan, 1 << 20, 17, 2) == (7, 1, 1, 8 << 23)
    assert _chunks(plan, 1 << 20, 17, 2, 16).tolist() == [[0, 1, 0, 7], [0, 1, 7, 7], [0, 1, 14, 3],
                                                            [1, 1, 0, 7], [1, 1, 7, 7], [1, 1, 14, 3]]
    # n = 512: 16384 frames fit; F = 3: 5461 groups a chunk
    assert _plan(plan, 512, 3, 70) == (3, 70, 0, 70 * 3 * 512 * 8)
    assert _chunks(plan, 512, 3, 6000, 4).tolist() == [[0, 5461, 0, 3], [5461, 539, 0, 3]]


@pytest.mark.parametrize("n,channels", [(8, 2), (512, 2), (8192, 2), (16, 1), (256, 1), (16384, 1)])
def test_launches_on_the_single_workgroup_sizes_do_not_grow_with_the_groups(plan, n, channels):
    """Two launches per chunk -- the transform of all its groups' frames and the reduce -- so a call that fits the
    scratch area takes two launches for 1 group and for 256, and a call that does not takes two per chunk: the count
    follows the bytes, never the groups."""
    assert plan.spec_avg_path(n, channels) == WR_FFT_SINGLE
    cap = plan.spec_avg_cap_bytes()
    for F in FS:
        one, many = plan.spec_avg_launches(n, channels, F, 1), plan.spec_avg_launches(n, channels, F, 256)
        if 256 * F * n * 8 <= cap:
            assert one == many == 2, (n, F)
        assert one == 2 * len(_chunks(plan, n, F, 1, 1000))
        assert many == 2 * len(_chunks(plan, n, F, 256, 450_000))


def test_launches_on_the_two_pass_sizes_loop_over_the_groups(plan):
    """65536 IQ points: F = 5 in 3 groups is one chunk: per group pass 1 and pass 2, then the reduce.  A real plan has the
    untangle step too.  F = 259 does not fit the scratch area's 128 frames: chunks of 127 frames and the carry."""
    assert plan.spec_avg_path(65536, 2) != WR_FFT_SINGLE
    assert plan.spec_avg_launches(65536, 2, 5, 3) == 3 * 2 + 1
    assert plan.spec_avg_launches(32768, 1, 5, 3) == 3 * 3 + 1
    if plan.spec_avg_cap_bytes() == 64 << 20:
        assert _chunks(plan, 65536, 259, 1, 8)[:, 3].tolist() == [127, 127, 5]
        assert plan.spec_avg_launches(65536, 2, 259, 1) == 3 * (2 + 1)
