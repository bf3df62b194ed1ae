"""-m gpu: the voice bank -- wr_voice_push_rows on plain rows and wr_tuner_voice_push behind a tuner -- BIT FOR BIT against the
numpy restatement of the header's rule (tests/voice_np.py, held to the rule's plain loops, to an ideal delayed sine and to
a unit-impulse filter in test_voice_capi.py): every output frame of every row after every push, from the very floats
uploaded; a sentinel NaN shows that nothing beside the output rows was written.

The taps are seeded random ones up to +-16 with -0.0, subnormals and 16.0 among them: what is compared is the arithmetic,
which does not care what the taps mean.  The chunk of outputs a workgroup takes and the outputs a thread takes are the
plan's (wr_plan.h's VOICE_CHUNK and VOICE_PER through tests/launch_plan.py), and the pushes are cut around them.

The tuner test is the tone bank's: FS 2 MHz, channel rate 5 kHz, audio 1 kHz with five NFM receivers (tones_np.fm_block),
twelve submits of 100 000 frames = 50 audio frames each, through a bank of 64 rows of 64 taps -- a history longer than a
block -- and on into a Resampler at 1 000 -> 750 Hz (3 / 4, P = 32)."""
import ctypes as C

import numpy as np
import pytest

import launch_plan
import resamp_np
import rowcases
import tones_np
import voice_np
from rowcases import BLOCK, K2, NBLOCKS, SENTINEL, fm_stream  # noqa: F401  (fm_stream: the fixture)
from voice_np import MUTE
from webradio_amd import capi
from webradio_amd.device import Resampler, VoiceBank

pytestmark = pytest.mark.gpu

SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, -0.0, 1e-40, 65536.0]


CHUNKS = [launch_plan.voice_plan().chunk]                                 # outputs a workgroup takes
PERS = [launch_plan.voice_plan().per]                                     # ... and a thread


def _taps(F, T, seed):
    taps = np.random.default_rng(seed).uniform(-16.0, 16.0, (F, T)).astype(np.float32)
    taps[0, 0], taps[1 % F, 3], taps[F - 1, T - 1], taps[F - 1, 2], taps[0, T // 2] = -0.0, 1e-40, -1e-42, 16.0, -16.0
    return taps


def _rows(nrows, n, seed):
    """values from 1e-4 to beyond the clamp, both signs, and in every row the non-finite, saturating, signed-zero and
    subnormal values"""
    return rowcases.special_rows(nrows, n, seed, 7, SPECIAL)


def _push(dev, bank, want, p_in, stride, nrows, pos, length, v, what):
    """one push of frames [pos, pos + length) of the first nrows rows, compared: every output bit, and nothing written
    beside the rows"""
    _, check = rowcases.padded_push(dev, nrows, length, lambda p_out, ostride: bank.push_rows(p_in + 4 * pos, stride, nrows, length,
                                                                                          p_out, ostride), what)
    ref = want.push(v[:nrows, pos: pos + length])
    check(ref)
    return ref


# ---- 1: plain rows, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T, nrows", [(8, 1), (8, 3), (8, 65), (64, 3), (64, 65), (1024, 3), (2048, 1), (2048, 3)])
def test_rows_against_the_restatement(dev, T, nrows):
    """F = 3, row r on filter r % 3, row 1 muted where there is one.  The pushes: 1 frame, T - 2, T - 1 (shorter than the
    history: the new history holds old history), none, PER - 1 for every PER (a thread's outputs one short), and for every
    chunk size C: C - 1 (a chunk one output short), C (full), C + 1 (a second chunk of one output); then 300."""
    F = 3
    lengths = [1, T - 2, T - 1, 0] + [per - 1 for per in PERS]
    for c in CHUNKS:
        lengths += [c - 1, c, c + 1]
    lengths.append(300)
    n = sum(lengths)
    taps = _taps(F, T, seed=T + nrows)
    v = _rows(nrows, n, seed=1000 * nrows + T)
    words = np.arange(nrows, dtype=np.uint32) % F
    if nrows > 1:
        words[1] |= MUTE
    want = voice_np.Bank(nrows, taps)
    want.set_rows(0, words)
    bank = VoiceBank(dev, nrows, taps)
    p, p0, stride = rowcases.upload_laid_out(dev, v)
    try:
        assert bank.info() == (T, F, 0) and not bank.get_rows().any()
        bank.set_rows(0, words)
        assert np.array_equal(bank.get_rows(), words)
        pos, loud = 0, 0.0
        for length in lengths:
            ref = _push(dev, bank, want, p0, stride, nrows, pos, length, v, (T, nrows, pos, length))
            pos += length
            if length:
                loud = max(loud, float(np.abs(ref[0]).max()))
                assert nrows == 1 or not ref[1].view(np.uint32).any()        # the muted row: +0.0f
        assert loud > 0
        assert bank.info() == (T, F, n) and want.frames == n
    finally:
        bank.destroy()
        dev.free(p)


def test_several_chunks_a_row_and_a_rest_of_twelve_taps(dev):
    """65 rows of three and more chunks each, so that workgroups in the middle of a row take their whole span from the push,
    with 28 taps: a turn of sixteen and a rest of twelve, which no length of the test above has"""
    T, F, nrows, C = 28, 3, 65, CHUNKS[-1]
    lengths = [3 * C - 1, 3 * C, 3 * C + 1, T - 2, 300, 5 * C + 17]
    n = sum(lengths)
    taps = _taps(F, T, seed=99)
    v = _rows(nrows, n, seed=98)
    words = np.arange(nrows, dtype=np.uint32) % F
    words[1] |= MUTE
    want = voice_np.Bank(nrows, taps)
    want.set_rows(0, words)
    bank = VoiceBank(dev, nrows, taps)
    p, p0, stride = rowcases.upload_laid_out(dev, v)
    try:
        bank.set_rows(0, words)
        pos = 0
        for length in lengths:
            _push(dev, bank, want, p0, stride, nrows, pos, length, v, ("chunks", pos, length))
            pos += length
        assert bank.info() == (T, F, n)
    finally:
        bank.destroy()
        dev.free(p)


# ---- 2: reset, rows left out, controls ------------------------------------------------------------------------------------------

def test_reset_rows_left_out_and_controls(dev):
    T, F, nrows, n = 64, 3, 4, 500
    taps = _taps(F, T, seed=5)
    v = _rows(nrows, n, seed=6)
    bank, want = VoiceBank(dev, nrows, taps), voice_np.Bank(nrows, taps)
    p, p0, stride = rowcases.upload_laid_out(dev, v)
    lib = dev.lib

    def words(first, w):
        bank.set_rows(first, w)
        want.set_rows(first, w)
        assert np.array_equal(bank.get_rows(), want.ctl)

    def refused(first, w):
        w = np.asarray(w, np.uint32)
        assert lib.wr_voice_set_rows(bank.h, first, w.size, capi.ptr(w)) == capi.WR_ERR_ARG
        assert b"wr_voice_set_rows" in lib.wr_last_error()
        assert np.array_equal(bank.get_rows(), want.ctl)                    # ... and no word changed

    try:
        words(0, [0, 1, 2, 1 | MUTE])
        _push(dev, bank, want, p0, stride, nrows, 0, 100, v, "first")
        # a reset of one row in mid-stream clears that row only; its control word stays
        bank.reset(2)
        want.reset(2)
        assert np.array_equal(bank.get_rows(), want.ctl)
        _push(dev, bank, want, p0, stride, nrows, 100, 7, v, "row 2 reset")   # (shorter than the history)
        assert bank.info()[2] == 107
        # a push of fewer rows clears the rows it leaves out: rows 2 and 3 saw nothing
        _push(dev, bank, want, p0, stride, 2, 107, 50, v, "two of four")
        assert not want.hist[2:].any()
        _push(dev, bank, want, p0, stride, nrows, 157, 60, v, "four again")
        # ... also when the pushes of fewer rows alternate with a reset in between
        _push(dev, bank, want, p0, stride, 3, 217, 20, v, "three")
        bank.reset(0)
        want.reset(0)
        _push(dev, bank, want, p0, stride, nrows, 237, 14, v, "four, row 0 reset")
        # a filter index changed between pushes: the new taps meet the old inputs; mute on, and off again: the history ran on
        words(0, [2])
        words(2, [2 | MUTE, 1])
        _push(dev, bank, want, p0, stride, nrows, 251, 30, v, "row 0 on filter 2, row 2 muted, row 3 speaks")
        words(1, [0, 0])
        ref = _push(dev, bank, want, p0, stride, nrows, 281, 40, v, "row 2 speaks again")
        assert np.abs(ref[2]).max() > 0
        # refused: an index that is not below F, a stray bit, rows beyond the bank -- the whole call, its good words too
        refused(0, [1, 3])
        refused(1, [2, 0x200 | 1])
        refused(2, [0, 1 << 31])
        refused(3, [0, 0])
        refused(5, [])
        _push(dev, bank, want, p0, stride, nrows, 321, 29, v, "behind the refused calls")
        # reset of all rows: every history cleared, the frame count back at 0, the control words as they were
        bank.reset()
        want.reset()
        assert bank.info() == (T, F, 0) and np.array_equal(bank.get_rows(), want.ctl)
        _push(dev, bank, want, p0, stride, nrows, 350, 150, v, "after the reset of all")
        assert bank.info() == (T, F, 150)
    finally:
        bank.destroy()
        dev.free(p)


# ---- 3: behind a tuner ----------------------------------------------------------------------------------------------------------

OUT_RATE, RS_TAPS, VT = 750, 32, 64


def _raw_push(dev, t, bank, stride, out=True):
    """wr_tuner_voice_push into a buffer of 64 rows of `stride` floats (out False: a NULL out_dev); (rc, slots, the rows)"""
    slots = C.c_uint()
    rc, got = rowcases.raw_tuner_push(dev, lambda p, s: dev.lib.wr_tuner_voice_push(t.h, bank.h, p, s, C.byref(slots)), stride, out)
    return rc, slots.value, got


@pytest.mark.parametrize("streaming", [False, True], ids=["per-block", "streaming"])
def test_behind_a_tuner(dev, fm_stream, streaming):
    x = fm_stream
    plain = rowcases.twin_audio(dev, x, capi.WR_NCO_ROTATE, streaming)   # the same tuner that never sees the call
    t, chans = rowcases.fm_tuner(dev, capi.WR_NCO_ROTATE, streaming)
    slots = [t.slot(ch) for ch in chans]
    taps = _taps(2, VT, seed=31)
    bank, want = VoiceBank(dev, 64, taps), voice_np.Bank(64, taps)
    rs = Resampler(dev, 64, tones_np.AUDIO_RATE, OUT_RATE, RS_TAPS)
    rs_want = resamp_np.Bank(64, rs.L, rs.M, rs.taps)
    assert (rs.L, rs.M, rs.P) == (3, 4, 32) and VT - 1 > K2
    words = np.zeros(64, np.uint32)
    words[slots] = np.arange(len(slots)) % 2
    bank.set_rows(0, words)
    want.set_rows(0, words)
    stride = K2 + 3
    p_out = dev.upload(np.full(64 * stride, SENTINEL, np.float32))
    p_rs = dev.malloc(64 * K2 * 4)
    try:
        for b in range(NBLOCKS):
            if b == 6:                                                      # one receiver muted from block 6 on
                bank.set_rows(slots[2], [words[slots[2]] | MUTE])
                want.set_rows(slots[2], [words[slots[2]] | MUTE])
            t.submit_device(x + 8 * BLOCK * b, BLOCK)
            if streaming and b % 2:
                assert t.stream_info()[0] is True
            assert t.voice_push(bank, p_out, stride) == 64
            assert t.stream_info()[0] is False                             # the getter closed the open launch
            got = dev.download(p_out, 64 * stride).reshape(64, stride)
            assert np.all(got[:, K2:].view(np.uint32) == SENTINEL.view(np.uint32))
            rows = t.fetch_audio_all()
            assert rows.shape == (64, K2)
            for c, ch in enumerate(chans):
                # the push changes no audio bit of the tuner
                assert np.array_equal(rows[slots[c]].view(np.uint32), plain[b][c].view(np.uint32)), (b, c)
            ref = want.push(rows)
            # (rows of slots without a channel carry no meaning: compared are the five receivers' rows)
            assert np.array_equal(got[slots, :K2].view(np.uint32), ref[slots].view(np.uint32)), b
            if b >= 6:
                assert not got[slots[2], :K2].view(np.uint32).any()
            # the output is a plain block of rows: straight on into the resampler
            n_out = rs.push_rows(p_out, stride, 64, K2, p_rs, K2)
            rs_ref = rs_want.push(ref)
            rs_got = dev.download(p_rs, 64 * K2).reshape(64, K2)[:, :n_out]
            assert n_out == rs_ref.shape[1]
            assert np.array_equal(rs_got[slots].view(np.uint32), rs_ref[slots].view(np.uint32)), b
        assert np.abs(ref[slots]).max() > 0 and np.abs(rs_ref[slots]).max() > 0
        assert bank.info() == (VT, 2, NBLOCKS * K2)
    finally:
        dev.free(p_out)
        dev.free(p_rs)
        rs.destroy()
        bank.destroy()
        t.destroy()


# ---- 4: tuner errors -------------------------------------------------------------------------------------------------------------

def test_tuner_errors_and_a_slot_taken_again(dev, fm_stream):
    lib = dev.lib
    t, chans = rowcases.fm_tuner(dev, capi.WR_NCO_ROTATE)
    taps = _taps(2, VT, seed=32)
    bank, small, want = VoiceBank(dev, 64, taps), VoiceBank(dev, 5, taps), voice_np.Bank(64, taps)
    slots = [t.slot(ch) for ch in chans]
    stride = K2 + 1

    def good_push(b):
        t.submit_device(fm_stream + 8 * BLOCK * b, BLOCK)
        rc, used, got = _raw_push(dev, t, bank, stride)
        assert rc == capi.WR_OK and used == 64
        ref = want.push(t.fetch_audio_all())
        assert np.array_equal(got[slots, :K2].view(np.uint32), ref[slots].view(np.uint32)), b
        return ref

    try:
        assert _raw_push(dev, t, bank, stride)[0] == capi.WR_ERR_STATE          # nothing submitted yet
        assert b"wr_tuner_voice_push" in lib.wr_last_error()
        t.submit_device(fm_stream, BLOCK)
        assert _raw_push(dev, t, small, stride)[0] == capi.WR_ERR_ARG           # 64 slots, 5 rows
        assert b"wr_tuner_voice_push" in lib.wr_last_error()
        rc, _, got = _raw_push(dev, t, bank, K2 - 1)                            # out_stride below the frames, several rows
        assert rc == capi.WR_ERR_ARG and np.all(got.view(np.uint32) == SENTINEL.view(np.uint32))
        assert _raw_push(dev, t, bank, stride, out=False)[0] == capi.WR_ERR_ARG  # a NULL out_dev
        a, a_stride, a_frames = t.audio_dev()
        assert a_frames == K2
        u = C.c_uint()
        assert lib.wr_tuner_voice_push(t.h, bank.h, C.c_void_p(a), a_stride, C.byref(u)) == capi.WR_ERR_ARG
        assert b"overlap" in lib.wr_last_error()                               # the tuner's own audio rows as the output
        assert bank.info()[2] == 0                                              # the refused pushes counted nothing
        rc, used, got = _raw_push(dev, t, bank, stride)
        ref = want.push(t.fetch_audio_all())
        assert rc == capi.WR_OK and np.array_equal(got[slots, :K2].view(np.uint32), ref[slots].view(np.uint32))
        assert _raw_push(dev, t, bank, stride)[0] == capi.WR_ERR_STATE          # the same submit twice
        assert b"already" in lib.wr_last_error()
        assert bank.info()[2] == K2                                             # ... and nothing was counted twice
        good_push(1)
        # a receiver removed and another added into the same slot: its row restarts from silence once the caller resets it
        gone = slots[2]
        t.remove_receiver(chans[2])
        ch = t.add_receiver(100_077, tones_np.CHAN_PASSBAND, tones_np.CHAN_RATE, capi.WR_FM, tones_np.AUDIO_PASSBAND,
                            tones_np.AUDIO_RATE)
        assert t.slot(ch) == gone
        assert want.hist[gone].any()
        bank.reset(gone)
        want.reset(gone)
        for b in (2, 3):
            ref = good_push(b)
        assert np.abs(ref[gone]).max() > 0
    finally:
        bank.destroy()
        small.destroy()
        t.destroy()


# ---- 5: argument errors ----------------------------------------------------------------------------------------------------------

def test_argument_errors(dev):
    lib = dev.lib
    h = C.c_void_p()

    def create(max_rows, T, F, taps):
        return lib.wr_voice_create(C.byref(h), dev.h, max_rows, T, F, capi.ptr(np.ascontiguousarray(taps, np.float32)))

    big = np.zeros((17, 2052), np.float32)
    good = _taps(2, 16, seed=1)
    for what, rc in [("T %d" % T, create(4, T, 2, big)) for T in (0, 4, 6, 2052)] + [
            ("F 0", create(4, 16, 0, big)), ("F 17", create(4, 16, 17, big)), ("rows 0", create(0, 16, 2, good)),
            ("rows 65536", create(65536, 16, 2, good)), ("nan", create(4, 16, 2, np.where(np.arange(32).reshape(2, 16) == 31, np.nan, good))),
            ("inf", create(4, 16, 2, np.where(np.arange(32).reshape(2, 16) == 0, np.inf, good))),
            ("17", create(4, 16, 2, np.where(np.arange(32).reshape(2, 16) == 5, 17.0, good))),
            ("-17", create(4, 16, 2, np.where(np.arange(32).reshape(2, 16) == 20, -17.0, good)))]:
        assert rc == capi.WR_ERR_ARG, what
        assert b"wr_voice_create" in lib.wr_last_error(), what
    bank = VoiceBank(dev, 2, good)
    p = dev.upload(np.zeros(256, np.float32))
    q = dev.upload(np.zeros(256, np.float32))

    def push(src, stride, nrows, nframes, dst, ostride):
        return lib.wr_voice_push_rows(bank.h, C.c_void_p(src), stride, nrows, nframes, C.c_void_p(dst) if dst else None, ostride)

    try:
        for what, rc in (("nrows > max_rows", push(p, 50, 3, 50, q, 50)), ("rows that overlap", push(p, 49, 2, 50, q, 50)),
                         ("output rows that overlap", push(p, 50, 2, 50, q, 49)), ("NULL out_dev", push(p, 50, 2, 50, None, 50)),
                         ("input and output: the same rows", push(p, 50, 2, 50, p, 50)),
                         ("the output begins at the input's last frame", push(p, 50, 2, 50, p + 4 * 99, 50)),
                         ("2^28 + 1 frames", push(p, 0, 1, (1 << 28) + 1, q, 0))):
            assert rc == capi.WR_ERR_ARG, what
            assert b"wr_voice_push_rows" in lib.wr_last_error(), what
        assert push(p, 50, 2, 50, p, 50) == capi.WR_ERR_ARG and b"overlap" in lib.wr_last_error()
        assert lib.wr_voice_reset(bank.h, 2) == capi.WR_ERR_ARG and b"wr_voice_reset" in lib.wr_last_error()
        assert bank.info()[2] == 0                                              # the refused pushes counted nothing
        assert push(p + 4 * 50, 50, 1, 50, p, 50) == capi.WR_OK                 # the output ends just in front of the input
        assert push(p, 49, 1, 50, q, 1) == capi.WR_OK                           # one row: any strides
        assert bank.info()[2] == 100
        calls = lib.wr_block_kernel_calls()
        assert push(p, 50, 2, 50, q, 50) == capi.WR_OK and lib.wr_block_kernel_calls() == calls + 1
        dev.sync()
    finally:
        bank.destroy()
        dev.free(p)
        dev.free(q)
