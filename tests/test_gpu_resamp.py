"""-m gpu: the resampler -- wr_resamp_push_rows on plain rows and wr_tuner_resamp_push behind a tuner -- BIT FOR BIT against the
numpy restatement of the header's rule (tests/resamp_np.py, held to the rule's plain loops and to an ideal delayed sine in
test_resamp_capi.py): every output frame of every row and the output count after every push, from the very floats uploaded.

The taps are wr_resamp_design's own wherever it makes any.  It refuses three of the shapes below -- P = 4 and P = 8 leave no
passband at any ratio (min(in, out) > 10 in / P cannot hold), and neither does 1 / 8 at P = 64 -- so those three run on
seeded random taps in +-1: what is compared is the arithmetic, which does not care what the taps mean.

The tuner test is the tone bank's: FS 2 MHz, channel rate 5 kHz, audio 1 kHz with five NFM receivers (tones_np.fm_block),
twelve submits of 100 000 frames = 50 audio frames each, through a bank of 64 rows at 1 000 -> 750 Hz (3 / 4, P = 32)."""
import ctypes as C

import numpy as np
import pytest

import resamp_np
import rowcases
import tones_np
from rowcases import BLOCK, K2, NBLOCKS, SENTINEL, SPECIAL, fm_stream  # noqa: F401  (fm_stream: the fixture)
from webradio_amd import capi
from webradio_amd.device import Resampler, resamp_design

pytestmark = pytest.mark.gpu

# (L, M, P) -> the rates wr_resamp_design is asked for; None: it makes no taps for this shape (see above)
SHAPES = {(3, 2, 4): None, (24, 25, 32): (50_000, 48_000), (24, 125, 64): (250_000, 48_000), (441, 500, 32): (50_000, 44_100),
          (1, 1, 8): None, (8, 1, 16): (6_000, 48_000), (1, 8, 64): None}


def _taps(L, M, P):
    rates = SHAPES[(L, M, P)]
    if rates is None:
        return np.random.default_rng(100 * L + P).uniform(-1.0, 1.0, (L, P)).astype(np.float32)
    taps, l, m = resamp_design(rates[0], rates[1], P)
    assert (l, m) == (L, M)
    return taps


def _bank(dev, max_rows, L, M, taps):
    """a Resampler of ratio L / M on these taps (the rates are only the ratio's)"""
    return Resampler(dev, max_rows, M, L, taps=taps)


def _rows(nrows, n, seed):
    """values from 1e-4 to beyond the clamp, both signs, and in every row the non-finite, saturating, signed-zero and
    subnormal values"""
    return rowcases.special_rows(nrows, n, seed, 7, SPECIAL)


def _frames_for(want, outputs):
    """the shortest push that yields at least `outputs` frames now (exactly that many unless L > M makes them come in runs)"""
    n = max(outputs * want.M // want.L - 2, 0)
    while want.out_frames(n) < outputs:
        n += 1
    return n


def _push(dev, rs, want, p_in, stride, nrows, pos, length, v, what):
    """one push of frames [pos, pos + length) of every row, compared: the count foretold, every output bit, and nothing
    written beside the rows"""
    n_want = want.out_frames(length)
    assert rs.out_frames(length) == n_want, what
    n_out, check = rowcases.padded_push(dev, nrows, n_want, lambda p_out, ostride: rs.push_rows(p_in + 4 * pos, stride, nrows, length,
                                                                                            p_out, ostride), what)
    ref = want.push(v[:nrows, pos: pos + length])
    assert n_out == n_want == ref.shape[1], (what, n_out, n_want)
    check(ref)
    return n_out


# ---- 1: plain rows, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L, M, P", list(SHAPES))
@pytest.mark.parametrize("nrows", [1, 3, 64, 65])
def test_rows_against_the_restatement(dev, nrows, L, M, P):
    taps = _taps(L, M, P)
    want = resamp_np.Bank(nrows, L, M, taps)
    # the pushes: 1 frame, P - 2, P - 1 (shorter than the history: the new history holds old history), one frame that yields
    # nothing (L < M), exactly 255, 256 and 257 outputs (one workgroup short, full, and a second one of one output),
    # 3 000 frames
    plan = resamp_np.Bank(1, L, M, taps)
    lengths = []

    def add(n):
        lengths.append(n)
        plan.push(np.zeros((1, n), np.float32))

    for n in (1, P - 2, P - 1):
        add(n)
    if L < M:
        while plan.out_frames(1):
            add(1)
        add(1)
    for outputs in (255, 256, 257):
        add(_frames_for(plan, outputs))
    add(3000)
    n = sum(lengths)
    v = _rows(nrows, n, seed=1000 * nrows + 10 * L + P)
    rs = _bank(dev, nrows, L, M, taps)
    p, p0, stride = rowcases.upload_laid_out(dev, v)
    try:
        pos, counts = 0, []
        for length in lengths:
            counts.append(_push(dev, rs, want, p0, stride, nrows, pos, length, v, (nrows, L, M, P, pos, length)))
            pos += length
        assert 0 in counts or L >= M
        if L <= M:
            assert {255, 256, 257} <= set(counts)
        assert rs.info() == (L, M, P, n, sum(counts)) and sum(counts) == resamp_np.ceil_div(n * L, M)
    finally:
        rs.destroy()
        dev.free(p)


def test_rough_taps(dev):
    """random taps up to +-16 with -0.0 and subnormals among them"""
    L, M, P, nrows = 7, 5, 12, 3
    rng = np.random.default_rng(77)
    taps = rng.uniform(-16.0, 16.0, (L, P)).astype(np.float32)
    taps[0, 0], taps[1, 3], taps[4, 7], taps[2, 2], taps[6, 11], taps[3, 0] = -0.0, 1e-40, -1e-42, 16.0, -16.0, 0.0
    n = 700
    v = _rows(nrows, n, seed=78)
    rs, want = _bank(dev, nrows, L, M, taps), resamp_np.Bank(nrows, L, M, taps)
    p = dev.upload(v.reshape(-1))
    try:
        pos = 0
        for length in (5, 11, 400, n - 416):
            _push(dev, rs, want, p, n, nrows, pos, length, v, ("rough", pos))
            pos += length
    finally:
        rs.destroy()
        dev.free(p)


# ---- 2: reset and rows left out -------------------------------------------------------------------------------------------------

def test_reset_and_rows_left_out(dev):
    L, M, P, nrows, n = 24, 25, 32, 4, 400
    taps = _taps(L, M, P)
    v = _rows(nrows, n, seed=5)
    rs, want = _bank(dev, nrows, L, M, taps), resamp_np.Bank(nrows, L, M, taps)
    p = dev.upload(v.reshape(-1))
    try:
        _push(dev, rs, want, p, n, nrows, 0, 100, v, "first")
        # a reset of one row in mid-stream clears that row only: the clock runs on
        rs.reset(2)
        want.reset(2)
        _push(dev, rs, want, p, n, nrows, 100, 7, v, "row 2 reset")           # (shorter than the history)
        assert rs.info()[3:] == (107, want.frames_out)
        # a push of fewer rows clears the rows it leaves out: rows 2 and 3 saw nothing
        _push(dev, rs, want, p, n, 2, 107, 50, v, "two of four")
        assert not want.hist[2:].any()
        _push(dev, rs, want, p, n, nrows, 157, 60, v, "four again")
        # ... also when the pushes of fewer rows alternate with a reset in between
        _push(dev, rs, want, p, n, 3, 217, 20, v, "three")
        rs.reset(0)
        want.reset(0)
        _push(dev, rs, want, p, n, nrows, 237, 14, v, "four, row 0 reset")
        assert want.nmod == 251 % M == 1
        # reset of all rows: every history cleared, the clock back at 0
        rs.reset()
        want.reset()
        assert rs.info() == (L, M, P, 0, 0) and rs.out_frames(1) == 1
        _push(dev, rs, want, p, n, nrows, 251, 149, v, "after the reset of all")
        assert rs.info() == (L, M, P, 149, 144)
    finally:
        rs.destroy()
        dev.free(p)


# ---- 3: behind a tuner ----------------------------------------------------------------------------------------------------------

OUT_RATE, TAPS = 750, 32


def _raw_push(dev, t, rs, stride):
    """wr_tuner_resamp_push into a buffer of 64 rows of `stride` floats; (rc, n_out, slots, the rows downloaded)"""
    n_out, slots = C.c_size_t(), C.c_uint()
    rc, got = rowcases.raw_tuner_push(dev, lambda p, s: dev.lib.wr_tuner_resamp_push(t.h, rs.h, p, s, C.byref(n_out), C.byref(slots)),
                                      stride)
    return rc, n_out.value, slots.value, got


@pytest.mark.parametrize("streaming", [False, True], ids=["per-block", "streaming"])
def test_behind_a_tuner(dev, fm_stream, streaming):
    x = fm_stream
    plain = rowcases.twin_audio(dev, x, capi.WR_NCO_ROTATE, streaming)   # the same tuner that never sees the call
    t, chans = rowcases.fm_tuner(dev, capi.WR_NCO_ROTATE, streaming)
    slots = [t.slot(ch) for ch in chans]
    rs = Resampler(dev, 64, tones_np.AUDIO_RATE, OUT_RATE, TAPS)
    want = resamp_np.Bank(64, rs.L, rs.M, rs.taps)
    assert (rs.L, rs.M, rs.P) == (3, 4, 32)
    calls = capi.load().wr_block_kernel_calls()
    try:
        for b in range(NBLOCKS):
            t.submit_device(x + 8 * BLOCK * b, BLOCK)
            n_want = want.out_frames(K2)
            if b % 2:
                if streaming:
                    assert t.stream_info()[0] is True
                rc, n_out, used, got = _raw_push(dev, t, rs, n_want + 3)
                assert rc == capi.WR_OK and used == 64 and n_out == n_want
                assert t.stream_info()[0] is False                             # the getter closed the open launch
                assert np.all(got[:, n_out:].view(np.uint32) == SENTINEL.view(np.uint32))
                got = got[:, :n_out]
            else:
                got = t.resamp_push(rs)
                assert got.shape == (64, n_want)
            rows = t.fetch_audio_all()
            assert rows.shape == (64, K2)
            for c, ch in enumerate(chans):
                # the resampler changes no audio bit of the tuner
                assert np.array_equal(rows[slots[c]].view(np.uint32), plain[b][c].view(np.uint32)), (b, c)
            ref = want.push(rows)
            # (rows of slots without a channel carry no meaning: compared are the five receivers' rows)
            assert np.array_equal(got[slots].view(np.uint32), ref[slots].view(np.uint32)), b
        assert np.abs(ref[slots]).max() > 0
        assert rs.info() == (3, 4, 32, NBLOCKS * K2, NBLOCKS * K2 * 3 // 4)
        assert capi.load().wr_block_kernel_calls() == calls                    # a getter, not a block-for-block call
    finally:
        rs.destroy()
        t.destroy()


def test_tuner_errors_and_a_new_slot(dev, fm_stream):
    lib = dev.lib
    t, chans = rowcases.fm_tuner(dev, capi.WR_NCO_ROTATE, spare=2)
    rs = Resampler(dev, 64, tones_np.AUDIO_RATE, OUT_RATE, TAPS)
    small = Resampler(dev, 5, tones_np.AUDIO_RATE, OUT_RATE, TAPS)
    want = resamp_np.Bank(64, rs.L, rs.M, rs.taps)
    try:
        assert _raw_push(dev, t, rs, 64)[0] == capi.WR_ERR_STATE                # nothing submitted yet
        assert b"wr_tuner_resamp_push" in lib.wr_last_error()
        t.submit_device(fm_stream, BLOCK)
        assert _raw_push(dev, t, small, 64)[0] == capi.WR_ERR_ARG               # 64 slots, 5 rows
        assert _raw_push(dev, t, rs, want.out_frames(K2) - 1)[0] == capi.WR_ERR_ARG   # out_stride below n_out
        got = t.resamp_push(rs)
        ref = want.push(t.fetch_audio_all())
        slots = [t.slot(ch) for ch in chans]
        assert np.array_equal(got[slots].view(np.uint32), ref[slots].view(np.uint32))
        assert _raw_push(dev, t, rs, 64)[0] == capi.WR_ERR_STATE                # the same submit twice
        assert b"already" in lib.wr_last_error()
        assert rs.info()[3:] == (K2, want.frames_out)                           # ... and nothing was counted twice
        # a receiver added into a new slot: its row starts from silence if the caller resets it
        ch = t.add_receiver(100_077, tones_np.CHAN_PASSBAND, tones_np.CHAN_RATE, capi.WR_FM, tones_np.AUDIO_PASSBAND,
                            tones_np.AUDIO_RATE)
        new = t.slot(ch)
        assert new not in slots
        rs.reset(new)
        want.reset(new)
        for b in (1, 2):
            t.submit_device(fm_stream + 8 * BLOCK * b, BLOCK)
            got = t.resamp_push(rs)
            ref = want.push(t.fetch_audio_all())
            assert np.array_equal(got[slots + [new]].view(np.uint32), ref[slots + [new]].view(np.uint32)), b
        # a second rate group
        t.add_receiver(50_000, tones_np.CHAN_PASSBAND, 10_000, capi.WR_FM, 2_000, 2_000)
        t.submit_device(fm_stream + 8 * BLOCK * 3, BLOCK)
        assert _raw_push(dev, t, rs, 64)[0] == capi.WR_ERR_STATE
        assert b"several rate groups" in lib.wr_last_error()
    finally:
        rs.destroy()
        small.destroy()
        t.destroy()


# ---- 4: errors ------------------------------------------------------------------------------------------------------------------

def test_argument_errors(dev):
    lib = dev.lib
    h = C.c_void_p()
    good = _taps(24, 25, 32)

    def create(max_rows, L, M, P, taps):
        return lib.wr_resamp_create(C.byref(h), dev.h, max_rows, L, M, P, capi.ptr(np.ascontiguousarray(taps, np.float32)))

    big = np.zeros((1025, 64), np.float32)
    for what, rc in (("inf", create(4, 24, 25, 32, np.where(np.arange(768).reshape(24, 32) == 5, np.inf, good))),
                     ("nan", create(4, 24, 25, 32, np.where(np.arange(768).reshape(24, 32) == 767, np.nan, good))),
                     ("17", create(4, 24, 25, 32, np.where(np.arange(768).reshape(24, 32) == 0, 17.0, good))),
                     ("-17", create(4, 24, 25, 32, np.where(np.arange(768).reshape(24, 32) == 9, -17.0, good))),
                     ("rows 0", create(0, 24, 25, 32, good)), ("rows 65536", create(65536, 24, 25, 32, good)),
                     ("L 0", create(4, 0, 25, 32, big)), ("L 1025", create(4, 1025, 1024, 4, big)),
                     ("M > 8 L", create(4, 1, 9, 32, big)), ("L > 8 M", create(4, 9, 1, 32, big)),
                     ("P 0", create(4, 3, 2, 0, big)), ("P 6", create(4, 3, 2, 6, big)), ("P 68", create(4, 3, 2, 68, big)),
                     ("L P", create(4, 441, 320, 64, big))):
        assert rc == capi.WR_ERR_ARG, what
        assert b"wr_resamp_create" in lib.wr_last_error()
    rs = _bank(dev, 2, 24, 25, good)
    p = dev.upload(np.zeros(256, np.float32))
    q = dev.upload(np.zeros(256, np.float32))
    n = C.c_size_t()

    def push(src, stride, nrows, nframes, dst, ostride):
        return lib.wr_resamp_push_rows(rs.h, C.c_void_p(src), stride, nrows, nframes, C.c_void_p(dst) if dst else None, ostride,
                                       C.byref(n))
    try:
        assert push(p, 50, 3, 50, q, 50) == capi.WR_ERR_ARG                     # nrows > max_rows
        assert push(p, 49, 2, 50, q, 50) == capi.WR_ERR_ARG                     # rows that overlap
        assert push(p, 50, 2, 50, q, 47) == capi.WR_ERR_ARG                     # out_stride below the 48 outputs
        assert push(p, 50, 2, 50, None, 50) == capi.WR_ERR_ARG
        assert push(p, 50, 2, 50, p, 50) == capi.WR_ERR_ARG                     # input and output: the same rows
        assert b"overlap" in lib.wr_last_error()
        assert push(p, 50, 2, 50, p + 4 * 99, 50) == capi.WR_ERR_ARG            # ... the output begins at the input's last frame
        assert push(p + 4 * 48, 50, 1, 50, p, 48) == capi.WR_OK                 # ... and ends just in front of it: no overlap
        assert n.value == 48
        assert lib.wr_resamp_reset(rs.h, 2) == capi.WR_ERR_ARG
        assert lib.wr_resamp_out_frames(rs.h, (1 << 28) + 1, C.byref(n)) == capi.WR_ERR_ARG
        assert rs.info()[3:] == (50, 48)                                        # the refused pushes moved no clock
        assert push(p, 49, 1, 50, q, 1) == capi.WR_OK                           # one row: any strides
        assert rs.info()[3:] == (100, 96)
        calls = lib.wr_block_kernel_calls()
        assert push(p, 50, 2, 50, q, 50) == capi.WR_OK and lib.wr_block_kernel_calls() == calls + 1
    finally:
        rs.destroy()
        dev.free(p)
        dev.free(q)
