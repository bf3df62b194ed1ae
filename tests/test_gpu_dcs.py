"""-m gpu: the DCS bank -- wr_dcs_push_rows on plain rows and wr_tuner_dcs_push behind a tuner -- BIT FOR BIT against the numpy
restatement of the header's rule (tests/dcs_np.py, held to the rule's plain loops in test_dcs_capi.py): agree, run, hits and
evals of every row after every push, from the very floats uploaded.

The tuner test is FS 2 MHz, channel rate 20 kHz, audio 5 kHz with six NFM receivers (dcs_np.fm_stream): four carry a code
(023, 754 inverted, 412, 131) under a 400 Hz tone of twice the deviation, one the 400 Hz tone alone, one is a bare carrier;
the bank has the 104 standard codes.  Ten blocks of 100 000 input frames are 2 500 audio frames: 67 evaluations, the first
22 of them without a full window of 23 bits."""
import ctypes as C

import numpy as np
import pytest

import dcs_np
import rowcases
from dcs_np import BLOCK, K2, NBLOCKS
from webradio_amd import DCS_CODES, capi
from webradio_amd.device import DcsBank, Tuner

pytestmark = pytest.mark.gpu

RATE = 5_000
SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, 64.0, -64.0, 64.5, -0.0, 0.0, 1e-40, -1e-40]
WORDS = [dcs_np.word(c) for c in DCS_CODES]
NAMES = ("agree", "run", "hits", "evals")


def _words(ncodes):
    """the standard codes' words, then 24 words of any weight (all zeros and all ones among them)"""
    extra = [0, 0x7FFFFF, 1, 0x2AAAAA] + [int(w) for w in np.random.default_rng(7).integers(0, 1 << 23, 20)]
    return (WORDS + extra)[:ncodes]


def _rows(n, rate, seed, noise=0.01):
    """[7][n]: four rows of normal deviates from 1e-4 to beyond the clamp with every awkward float among them, and three
    signal rows: a code as sent, a code inverted from a fractional bit, the voice tone alone"""
    v = rowcases.special_rows(4, n, seed, 3, SPECIAL)
    s = [dcs_np.signal_row(dcs_np.word(0o023), rate, n, seed + 1, start=0.37, noise=noise),
         dcs_np.signal_row(dcs_np.word(0o754), rate, n, seed + 2, start=7.9, inverted=True, noise=noise),
         dcs_np.signal_row(None, rate, n, seed + 3, noise=noise)]
    return np.concatenate([v, np.stack(s)])


def _same(bank, want, what, rows=slice(None)):
    got, ref = bank.read(), want.read()
    for g, r, name in zip(got, ref, NAMES):
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name)
        bad = np.argwhere(g[rows] != r[rows])
        assert bad.size == 0, (what, name, bad[:4], [int(g[rows][tuple(b)]) for b in bad[:4]],
                               [int(r[rows][tuple(b)]) for b in bad[:4]])
    return got


def _pair(dev, max_rows, words, rate, max_errors=0):
    bank = DcsBank(dev, max_rows, None, rate, max_errors, words=words)
    assert bank.step == dcs_np.step_of(rate)
    return bank, dcs_np.Bank(max_rows, words, bank.step, max_errors)


def _stream(dev, bank, want, v, lengths, stride_extra=0, lead=0, what=""):
    """pushes v[rows][n] cut into `lengths` (and the rest), rows `stride_extra` floats further apart than they are long
    behind `lead` floats; compares after every push"""
    nrows, n = v.shape
    stride = n + stride_extra
    buf = np.full(lead + nrows * stride, np.float32(np.nan), np.float32)      # (the gaps between rows are never read)
    for r in range(nrows):
        buf[lead + r * stride: lead + r * stride + n] = v[r]
    p = dev.upload(buf)
    try:
        pos = 0
        for length in list(lengths) + [n - sum(lengths)]:
            bank.push_rows(p + 4 * (lead + pos), stride, nrows, length)
            want.push(v[:, pos: pos + length])
            pos += length
            _same(bank, want, (what, pos))
        assert pos == n and bank.info()[3] == want.N
    finally:
        dev.free(p)


# ---- 1: plain rows, bit for bit -------------------------------------------------------------------------------------------------

def test_awkward_floats_and_cuts(dev):
    """pushes inside one chip (1, 7 frames), with no evaluation, with several; the same stream in one push gives the same"""
    n = 3_000
    v = _rows(n, RATE, seed=11)
    bank, want = _pair(dev, 7, WORDS, RATE)
    whole, want_whole = _pair(dev, 7, WORDS, RATE)
    try:
        _stream(dev, bank, want, v, [1, 7, 500, 501, 1_400], stride_extra=5, lead=1, what="cuts")
        _stream(dev, whole, want_whole, v, [], what="whole")
        for a, b, name in zip(bank.read(), whole.read(), NAMES):
            assert np.array_equal(a, b), name
        agree, run, hits, evals = bank.read()
        assert list(evals) == [80] * 7
        assert agree[4, DCS_CODES.index(0o023), 0] == 23 and run[4, DCS_CODES.index(0o023), 0] >= 8
        assert agree[5, DCS_CODES.index(0o754), 1] == 23 and run[5, DCS_CODES.index(0o754), 1] >= 8
        assert not run[6].any()
    finally:
        bank.destroy()
        whole.destroy()


@pytest.mark.parametrize("ncodes", [1, 64, 65, 128])
def test_code_counts(dev, ncodes):
    v = _rows(1_500, RATE, seed=20 + ncodes)
    bank, want = _pair(dev, 7, _words(ncodes), RATE)
    try:
        _stream(dev, bank, want, v, [700], what=ncodes)
        assert bank.read()[0].shape == (7, ncodes, 2) and bank.info()[0] == ncodes
        assert bank.read()[2][4, 0, 0] > 0                       # code 023 on its row
    finally:
        bank.destroy()


@pytest.mark.parametrize("max_errors", [0, 1, 2, 3])
def test_error_budget(dev, max_errors):
    """noise of the code's own amplitude: received words with one, two and more wrong bits"""
    v = _rows(2_000, RATE, seed=30, noise=0.05)
    bank, want = _pair(dev, 7, WORDS, RATE, max_errors)
    try:
        _stream(dev, bank, want, v, [999], what=max_errors)
        assert bank.info()[2] == max_errors
    finally:
        bank.destroy()


def test_two_frames_per_chip_and_more_chips_than_a_ring(dev):
    """2 151 Hz: a push of 40 000 frames is 20 000 chips -- many launches"""
    rate, n = 2_151, 40_000
    words = WORDS[:6] + [dcs_np.word(0o047), 0]
    v = np.stack([dcs_np.signal_row(words[0], rate, n, 41, start=5.5), dcs_np.signal_row(words[3], rate, n, 42, inverted=True)])
    bank, want = _pair(dev, 2, words, rate)
    try:
        _stream(dev, bank, want, v, [], what="2151 Hz")
        agree, run, hits, evals = bank.read()
        assert list(evals) == [((n * bank.step) >> 29) // 8] * 2 and evals[0] > 2_400
        assert hits[0, 0, 0] > 2_000 and hits[1, 3, 1] > 2_000
        # ... and in pushes that end inside a chip
        bank.reset()
        want.reset()
        _stream(dev, bank, want, v[:, :5_001], [1, 1, 1, 2_500, 1, 777], what="2151 Hz, cut")
    finally:
        bank.destroy()


def test_357_frames_per_bit(dev):
    rate, n = 48_000, 9_000
    v = np.stack([dcs_np.signal_row(WORDS[10], rate, n, 51, start=1.25), rowcases.special_rows(1, n, 52, 3, SPECIAL)[0]])
    bank, want = _pair(dev, 2, WORDS, rate)
    try:
        _stream(dev, bank, want, v, [4_000, 357, 44], stride_extra=3, what="48 kHz")
        agree, run, hits, evals = bank.read()
        assert list(evals) == [25, 25] and agree[0, 10, 0] == 23 and run[0, 10, 0] >= 2
    finally:
        bank.destroy()


def test_a_clock_beyond_2_to_the_64(dev):
    """seek(2^40 - 5): N * step passes 2^64 (step is about 2^26.8 at 5 kHz); the restatement's clock is a Python integer"""
    n = 2_000
    v = _rows(n, RATE, seed=60)
    bank, want = _pair(dev, 7, WORDS, RATE)
    try:
        for at in (2 ** 40 - 5, 2 ** 63 + 12_345, 2 ** 64 - n):                # (the last: N itself ends just below 2^64)
            bank.seek(at)
            want.seek(at)
            assert at * bank.step > 2 ** 64 and bank.info()[3] == at
            _same(bank, want, ("sought", at))
            assert not bank.read()[3].any()
            _stream(dev, bank, want, v[:, : n if at < 2 ** 64 - n else 1_300], [3, 600], what=at)
            assert bank.read()[3][0] > 30
    finally:
        bank.destroy()


# ---- 2: rows --------------------------------------------------------------------------------------------------------------------

def test_rows_left_out_are_reset(dev):
    n = 2_400
    v = _rows(n, RATE, seed=70)
    bank, want = _pair(dev, 7, WORDS, RATE)
    p = dev.upload(v.reshape(-1))
    try:
        bank.push_rows(p, n, 7, 1_200)
        want.push(v[:, :1_200])
        before = _same(bank, want, "all seven")
        assert before[3][6] == 32 and before[2][4].any()
        bank.push_rows(p + 4 * 1_200, n, 5, 600)                   # rows 5 and 6 are left out
        want.push(v[:5, 1_200:1_800])
        agree, run, hits, evals = _same(bank, want, "five of seven")
        assert list(evals) == [48] * 5 + [0, 0] and not agree[5:].any() and not run[5:].any() and not hits[5:].any()
        bank.push_rows(p + 4 * 1_800, n, 7, 600)                   # ... and begin new streams on the running clock
        want.push(v[:, 1_800:])
        agree, run, hits, evals = _same(bank, want, "seven again")
        assert list(evals) == [64] * 5 + [16, 16]
    finally:
        bank.destroy()
        dev.free(p)


def test_reset_clears_that_row_alone(dev):
    n = 2_400
    v = _rows(n, RATE, seed=80)
    bank, want = _pair(dev, 7, WORDS, RATE)
    p = dev.upload(v.reshape(-1))
    try:
        bank.push_rows(p, n, 7, 1_301)
        want.push(v[:, :1_301])
        before = [a.copy() for a in _same(bank, want, "before")]
        bank.reset(4)
        want.reset(4)
        after = _same(bank, want, "row 4 reset")
        keep = [0, 1, 2, 3, 5, 6]
        for a, b in zip(before, after):
            assert np.array_equal(a[keep], b[keep]) and not b[4].any()
        assert before[2][4].any() and bank.info()[3] == 1_301      # the clock goes on
        bank.push_rows(p + 4 * 1_301, n, 7, n - 1_301)
        want.push(v[:, 1_301:])
        agree, run, hits, evals = _same(bank, want, "after")
        assert list(evals[keep]) == [64] * 6 and evals[4] == 64 - 34
        bank.reset()
        want.reset()
        assert not any(a.any() for a in _same(bank, want, "all reset")) and bank.info()[3] == 0
    finally:
        bank.destroy()
        dev.free(p)


# ---- 3: behind a tuner ----------------------------------------------------------------------------------------------------------

def _tuner(dev, nco, spare=0):
    t = Tuner(dev, dcs_np.FS, len(dcs_np.IFS) + spare, BLOCK, nco)
    chans = [t.add_receiver(f, dcs_np.CHAN_PASSBAND, dcs_np.CHAN_RATE, capi.WR_FM, dcs_np.AUDIO_PASSBAND, dcs_np.AUDIO_RATE)
             for f in dcs_np.IFS]
    return t, chans


@pytest.fixture(scope="module")
def fm_stream(dev):
    """the ten blocks in device memory, back to back, uploaded once; twin(nco): [block][receiver] audio of the same tuner
    that never sees the call, a launch and a fetch per block, run once per NCO mode"""
    p = dev.upload(dcs_np.fm_stream())
    twins = {}

    def twin(nco):
        if nco not in twins:
            twins[nco] = rowcases.block_audio(_tuner(dev, nco), p, NBLOCKS, BLOCK, K2)
        return twins[nco]

    yield p, twin
    dev.free(p)


@pytest.mark.parametrize("how", ["per-block", "streaming"])
@pytest.mark.parametrize("nco", [capi.WR_NCO_EXACT, capi.WR_NCO_ROTATE], ids=["exact", "rotate"])
def test_behind_a_tuner(dev, fm_stream, nco, how):
    x, twin = fm_stream
    plain = twin(nco)
    t, chans = _tuner(dev, nco)
    if how == "streaming":
        t.streaming(True)
    slots = [t.slot(ch) for ch in chans]
    bank = DcsBank(dev, 64, DCS_CODES, dcs_np.AUDIO_RATE)
    want = dcs_np.Bank(64, bank.words, bank.step)
    assert list(bank.words) == WORDS
    try:
        for b in range(NBLOCKS):
            t.submit_device(x + 8 * BLOCK * b, BLOCK)
            assert t.dcs_push(bank) == 64
            assert t.stream_info()[0] is False                     # like every getter it closes an open streaming launch
            rows = np.zeros((64, K2), np.float32)
            for c, ch in enumerate(chans):
                a = t.fetch(ch, capi.WR_STAGE_AUDIO, K2)
                assert a.size == K2
                assert np.array_equal(a.view(np.uint32), plain[b][c].view(np.uint32)), (b, c)   # the bank changes no audio bit
                rows[slots[c]] = a
            want.push(rows)
            # (rows of slots without a channel carry no meaning: compared are the six receivers' rows)
            _same(bank, want, (how, b), rows=slots)
        agree, run, hits, evals = bank.read()
        assert list(evals[slots]) == [67] * 6 and bank.info()[3] == NBLOCKS * K2
        # the detection conditions on the GPU's own result
        own_runs, foreign = dcs_np.detection(agree, run, WORDS, slots)
        print("%s %s: own codes' run %s; largest run of any other code %d" % (
            "exact" if nco == capi.WR_NCO_EXACT else "rotate", how, own_runs, foreign))
    finally:
        bank.destroy()
        t.destroy()


# ---- 4: errors ------------------------------------------------------------------------------------------------------------------

def test_tuner_errors(dev, fm_stream):
    x, _ = fm_stream
    lib = dev.lib
    t, chans = _tuner(dev, capi.WR_NCO_ROTATE, spare=1)
    bank = DcsBank(dev, 64, DCS_CODES, dcs_np.AUDIO_RATE)
    small = DcsBank(dev, 6, DCS_CODES, dcs_np.AUDIO_RATE)
    try:
        assert lib.wr_tuner_dcs_push(t.h, bank.h, None) == capi.WR_ERR_STATE           # nothing submitted yet
        assert b"wr_tuner_dcs_push" in lib.wr_last_error()
        t.submit_device(x, BLOCK)
        assert lib.wr_tuner_dcs_push(t.h, small.h, None) == capi.WR_ERR_ARG            # 64 slots, 6 rows
        assert b"64 channel slots, the bank 6 rows" in lib.wr_last_error()
        assert t.dcs_push(bank) == 64
        assert lib.wr_tuner_dcs_push(t.h, bank.h, None) == capi.WR_ERR_STATE           # the same submit twice
        assert b"already" in lib.wr_last_error()
        assert bank.info()[3] == K2 and list(bank.read()[3][:1]) == [6]                # ... and nothing was counted twice
        t.submit_device(x + 8 * BLOCK, BLOCK)
        assert t.dcs_push(bank) == 64
        assert bank.info()[3] == 2 * K2
    finally:
        bank.destroy()
        small.destroy()
        t.destroy()


def test_argument_errors(dev):
    lib = dev.lib
    h = C.c_void_p()
    words = np.array(WORDS, np.uint32)
    step = dcs_np.step_of(RATE)
    for args in ((0, 104, step, 0), (65_536, 104, step, 0), (4, 0, step, 0), (4, 129, step, 0), (4, 104, (1 << 19) - 1, 0),
                 (4, 104, (1 << 28) + 1, 0), (4, 104, step, 4)):
        assert lib.wr_dcs_create(C.byref(h), dev.h, args[0], capi.ptr(words), *args[1:]) == capi.WR_ERR_ARG, args
        assert b"wr_dcs_create" in lib.wr_last_error() and b"(1 .. 65535)" in lib.wr_last_error()
    bad = np.array([5, 1 << 23], np.uint32)
    assert lib.wr_dcs_create(C.byref(h), dev.h, 4, capi.ptr(bad), 2, step, 0) == capi.WR_ERR_ARG
    assert b"not below 2^23" in lib.wr_last_error()
    bank, _ = _pair(dev, 2, WORDS[:2], RATE)
    p = dev.upload(np.zeros(64, np.float32))
    try:
        calls = dev.lib.wr_block_kernel_calls()
        assert lib.wr_dcs_push_rows(bank.h, C.c_void_p(p), 16, 3, 16) == capi.WR_ERR_ARG       # nrows > max_rows
        assert lib.wr_dcs_push_rows(bank.h, C.c_void_p(p), 15, 2, 16) == capi.WR_ERR_ARG       # rows that overlap
        assert lib.wr_dcs_push_rows(bank.h, C.c_void_p(p), 1 << 29, 2, (1 << 28) + 1) == capi.WR_ERR_ARG
        assert b"2^28" in lib.wr_last_error()
        assert lib.wr_dcs_push_rows(bank.h, None, 16, 2, 16) == capi.WR_ERR_ARG
        assert lib.wr_dcs_read(bank.h, None, None, None, None, None) == capi.WR_ERR_ARG
        assert lib.wr_dcs_reset(bank.h, 2) == capi.WR_ERR_ARG
        assert dev.lib.wr_block_kernel_calls() == calls
        assert lib.wr_dcs_push_rows(bank.h, C.c_void_p(p), 15, 1, 16) == capi.WR_OK            # one row: any stride
        assert dev.lib.wr_block_kernel_calls() == calls + 1                                    # counted as a block call
        assert bank.info() == (2, step, 0, 16)
        evals = np.zeros(2, np.uint64)
        assert lib.wr_dcs_read(bank.h, None, None, None, capi.ptr(evals), None) == capi.WR_OK   # any three may be NULL
        assert list(evals) == [0, 0]
    finally:
        bank.destroy()
        dev.free(p)
