"""-m gpu: the tone bank -- wr_tones_push_rows on plain rows and wr_tuner_tones_push behind a tuner -- BIT FOR BIT against the
numpy restatement of the header's rule (tests/tones_np.py, held to the rule's plain loops and to a float64 DFT in
test_tones_capi.py): I, Q, E, the window count and the fill of every row after every push, from the very floats uploaded.

The tuner test is FS 2 MHz, channel rate 5 kHz, audio 1 kHz with five NFM receivers (tones_np.fm_block): four carry a CTCSS
tone each (67.0, 100.0, 151.4, 254.1 Hz) plus a 400 Hz tone of twice the deviation, one the 400 Hz tone alone; the bank has
the 50 CTCSS tones and a window of 500 frames.  Blocks are 100 000 input frames = 50 audio frames, so the first window ends
in the tenth block: the test submits twelve (the bit comparison runs after each of them, the first six included), and a
second bank with a window of 120 frames on the same submits has window ends from the third block on."""
import ctypes as C

import numpy as np
import pytest

import rowcases
import tones_np
from rowcases import BLOCK, K2, NBLOCKS, fm_stream  # noqa: F401  (the fixture)
from webradio_amd import CTCSS_HZ, capi
from webradio_amd.device import ToneBank

pytestmark = pytest.mark.gpu

RATE = 1_000
SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, -0.0, 1e-40, 64.0]
NYQ = (1 << 31) - 1                                   # just below Nyquist: the phase wraps (nearly) every frame


def _steps(ntones):
    if ntones == 1:
        return np.array([NYQ], np.uint32)
    steps = [tones_np.step_of(hz, RATE) for hz in CTCSS_HZ]
    if ntones > 50:
        extra = np.random.default_rng(5).integers(1, 1 << 31, ntones - 50 - 4, dtype=np.int64)
        steps += [NYQ, NYQ - 12345, 1, 1 << 20] + [int(e) for e in extra]
    return np.array(steps[:ntones], np.uint32)


def _rows(nrows, n, seed):
    """values from 1e-4 to beyond the clamp, both signs, and in every row the non-finite and saturating values"""
    return rowcases.special_rows(nrows, n, seed, 3, SPECIAL)


def _lengths(W):
    """a push of 1 frame, several pushes per window, one that ends exactly on a window end, one equal to the window, one
    with two window ends (and frames behind them), one with three that ends exactly on the last, and a short tail"""
    return [1, W // 2 - 1, W - W // 2, W, 2 * W + 3, 3 * W - 3, W // 3]


def _same(bank, want, rows, what):
    iq, energy, windows, fill = bank.read()
    wiq, we, ww, wf = want.read()
    assert np.array_equal(windows[:rows], ww[:rows]), (what, windows[:rows], ww[:rows])
    assert np.array_equal(fill[:rows], wf[:rows]), (what, fill[:rows], wf[:rows])
    assert np.array_equal(energy[:rows], we[:rows]), what
    bad = np.argwhere(iq[:rows] != wiq[:rows])
    assert bad.size == 0, (what, bad[:4], [int(iq[tuple(b)]) for b in bad[:4]], [int(wiq[tuple(b)]) for b in bad[:4]])
    assert np.abs(iq).max() <= 1 << 46 and energy.max() <= 1 << 62
    return iq, energy, windows, fill


def _bank(dev, max_rows, steps, W):
    return ToneBank(dev, max_rows, None, None, W, steps=steps)


# ---- 1: plain rows, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [16, 17, 500])
@pytest.mark.parametrize("ntones", [1, 50, 64])
@pytest.mark.parametrize("nrows", [1, 3, 64, 65])
def test_rows_against_the_restatement(dev, nrows, ntones, W):
    lengths = _lengths(W)
    n = sum(lengths)
    # one row: back to back; three rows: an odd stride and a base one float off 16-byte alignment; 64 rows: a stride that
    # is a multiple of four frames and larger than the row; 65 rows: odd again
    extra, lead = {1: (0, 0), 3: (5, 1), 64: (8 - n % 4, 0), 65: (7, 1)}[nrows]
    stride = n + extra
    v = _rows(nrows, n, seed=1000 * nrows + 10 * ntones + W)
    buf = np.full(lead + nrows * stride, np.float32(np.nan), np.float32)      # (the gaps between rows are never read)
    for r in range(nrows):
        buf[lead + r * stride: lead + r * stride + n] = v[r]
    steps = _steps(ntones)
    bank = _bank(dev, nrows, steps, W)
    want = tones_np.Bank(nrows, steps, W)
    p = dev.upload(buf)
    try:
        pos = 0
        for length in lengths:
            bank.push_rows(p + 4 * (lead + pos), stride, nrows, length)
            want.push(v[:, pos: pos + length])
            pos += length
            _same(bank, want, nrows, (nrows, ntones, W, pos))
        assert int(want.windows[0]) == n // W >= 7
    finally:
        bank.destroy()
        dev.free(p)


def test_fewer_rows_than_the_bank_has(dev):
    """a push of two rows into a bank of four leaves rows 2 and 3 alone; a row pushed less often has its own fill"""
    W, n = 17, 40
    v = _rows(4, n, seed=3)
    steps = _steps(50)
    bank, want = _bank(dev, 4, steps, W), tones_np.Bank(4, steps, W)
    p = dev.upload(v.reshape(-1))
    try:
        bank.push_rows(p, n, 4, 25)
        want.push(v[:, :25])
        bank.push_rows(p + 4 * 25, n, 2, 15)
        want.push(v[:2, 25:])
        _, _, windows, fill = _same(bank, want, 4, "two of four")
        assert list(windows) == [2, 2, 1, 1] and list(fill) == [6, 6, 8, 8]
    finally:
        bank.destroy()
        dev.free(p)


def test_a_long_window_at_the_clamp(dev):
    """one row of W = 65536 frames of 64.0: E reaches its bound 2^62 and the tone that never leaves phase 0 its bound 2^46"""
    W = 65536
    steps = np.array([1, 65536, NYQ, tones_np.step_of(67.0, 48_000)], np.uint32)
    v = np.full((1, W + 700), 64.0, np.float32)
    bank, want = _bank(dev, 1, steps, W), tones_np.Bank(1, steps, W)
    p = dev.upload(v.reshape(-1))
    try:
        bank.push_rows(p, v.shape[1], 1, v.shape[1])
        want.push(v)
        iq, energy, windows, fill = _same(bank, want, 1, "W = 65536")
        assert int(energy[0]) == 1 << 62 and int(iq[0, 0, 0]) == 1 << 46 and int(iq[0, 0, 1]) == 0
        assert int(windows[0]) == 1 and int(fill[0]) == 700
    finally:
        bank.destroy()
        dev.free(p)


# ---- 2: reset -------------------------------------------------------------------------------------------------------------------

def test_reset_clears_that_row_alone(dev):
    W, n = 16, 60
    v = _rows(3, n, seed=4)
    steps = _steps(50)
    bank, want = _bank(dev, 3, steps, W), tones_np.Bank(3, steps, W)
    p = dev.upload(v.reshape(-1))
    try:
        bank.push_rows(p, n, 3, 41)
        want.push(v[:, :41])
        before = _same(bank, want, 3, "before")
        assert np.abs(before[0][1]).max() > 0 and int(before[2][1]) == 2 and int(before[3][1]) == 9
        bank.reset(1)
        want.reset(1)
        iq, energy, windows, fill = _same(bank, want, 3, "row 1 reset")
        assert not iq[1].any() and energy[1] == 0 and windows[1] == 0 and fill[1] == 0
        for a, b in zip(before, (iq, energy, windows, fill)):
            assert np.array_equal(a[[0, 2]], b[[0, 2]])
        # ... and the row begins a new stream: its windows are counted from the next frame pushed
        bank.push_rows(p + 4 * 41, n, 3, 19)
        want.push(v[:, 41:])
        _, _, windows, fill = _same(bank, want, 3, "after")
        assert list(windows) == [3, 1, 3] and list(fill) == [12, 3, 12]
        bank.reset()
        want.reset()
        iq, energy, windows, fill = _same(bank, want, 3, "all reset")
        assert not iq.any() and not energy.any() and not windows.any() and not fill.any()
    finally:
        bank.destroy()
        dev.free(p)


# ---- 3: behind a tuner ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["per-block", "streaming", "two-per-launch"])
@pytest.mark.parametrize("nco", [capi.WR_NCO_EXACT, capi.WR_NCO_ROTATE], ids=["exact", "rotate"])
def test_behind_a_tuner(dev, fm_stream, nco, how):
    x = fm_stream
    plain = rowcases.twin_audio(dev, x, nco)             # the same tuner with no bank, a launch per block
    t, chans = rowcases.fm_tuner(dev, nco)
    if how == "streaming":
        t.streaming(True)
    if how == "two-per-launch":
        t.blocks_per_launch(2)
    slots = [t.slot(ch) for ch in chans]
    hz = list(CTCSS_HZ)
    long_bank, short_bank = ToneBank(dev, 64, hz, tones_np.AUDIO_RATE, 500), ToneBank(dev, 64, hz, tones_np.AUDIO_RATE, 120)
    want = {500: tones_np.Bank(64, long_bank.steps, 500), 120: tones_np.Bank(64, short_bank.steps, 120)}
    try:
        for b in range(NBLOCKS):
            t.submit_device(x + 8 * BLOCK * b, BLOCK)
            if how == "streaming" and nco == capi.WR_NCO_ROTATE:
                assert t.stream_info()[0] is True                      # (EXACT tuners do not stream: the ordinary way)
            assert t.tones_push(long_bank) == 64
            assert t.stream_info()[0] is False
            assert t.tones_push(short_bank) == 64
            rows = np.zeros((64, K2), np.float32)
            for c, ch in enumerate(chans):
                a = t.fetch(ch, capi.WR_STAGE_AUDIO, K2)
                assert a.size == K2
                assert np.array_equal(a.view(np.uint32), plain[b][c].view(np.uint32)), (b, c)   # the bank changes no audio bit
                rows[slots[c]] = a
            for W, bank in ((500, long_bank), (120, short_bank)):
                want[W].push(rows)
                # (rows of slots without a channel carry no meaning: compared are the five receivers' rows)
                got, ref = bank.read(), want[W].read()
                for g, r, name in zip(got, ref, ("iq", "energy", "windows", "fill")):
                    assert np.array_equal(g[slots], r[slots]), (W, b, name)
        assert list(want[500].windows[slots]) == [1] * 5 and list(want[120].windows[slots]) == [5] * 5
        assert np.abs(want[500].iq[slots]).max() > 0
        # the detection conditions on the GPU's own latched window
        rho = long_bank.ratios()[slots]
        margins, untoned = tones_np.detection(rho, CTCSS_HZ)
        print("%s %s: own-tone rho %s; own / largest other %s; untoned largest / smallest own %.4g" % (
            "exact" if nco == capi.WR_NCO_EXACT else "rotate", how,
            ["%.4f" % rho[r, hz.index(f)] for r, f in enumerate(tones_np.TONED)], ["%.1f" % m for m in margins], untoned))
        assert min(margins) >= 4.0
        assert untoned < 0.25
    finally:
        long_bank.destroy()
        short_bank.destroy()
        t.destroy()


# ---- 4: errors ------------------------------------------------------------------------------------------------------------------

def test_tuner_errors(dev, fm_stream):
    lib = dev.lib
    t, chans = rowcases.fm_tuner(dev, capi.WR_NCO_ROTATE, spare=1)
    bank = ToneBank(dev, 64, CTCSS_HZ, tones_np.AUDIO_RATE, 500)
    small = ToneBank(dev, 5, CTCSS_HZ, tones_np.AUDIO_RATE, 500)
    try:
        assert lib.wr_tuner_tones_push(t.h, bank.h, None) == capi.WR_ERR_STATE         # nothing submitted yet
        assert b"wr_tuner_tones_push" in lib.wr_last_error()
        t.submit_device(fm_stream, BLOCK)
        assert lib.wr_tuner_tones_push(t.h, small.h, None) == capi.WR_ERR_ARG          # 64 slots, 5 rows
        assert t.tones_push(bank) == 64
        assert lib.wr_tuner_tones_push(t.h, bank.h, None) == capi.WR_ERR_STATE         # the same submit twice
        assert b"already" in lib.wr_last_error()
        assert list(bank.read()[3][:1]) == [K2]                                        # ... and nothing was counted twice
        t.submit_device(fm_stream + 8 * BLOCK, BLOCK)
        assert t.tones_push(bank) == 64
        # a second rate group
        t.add_receiver(50_000, tones_np.CHAN_PASSBAND, 10_000, capi.WR_FM, 2_000, 2_000)
        t.submit_device(fm_stream + 16 * BLOCK, BLOCK)
        assert lib.wr_tuner_tones_push(t.h, bank.h, None) == capi.WR_ERR_STATE
        assert b"several rate groups" in lib.wr_last_error()
    finally:
        bank.destroy()
        small.destroy()
        t.destroy()


def test_argument_errors(dev):
    lib = dev.lib
    h = C.c_void_p()
    ok = np.array([tones_np.step_of(100.0, RATE)] * 65, np.uint32)

    def create(max_rows, steps, ntones, window):
        return lib.wr_tones_create(C.byref(h), dev.h, max_rows, capi.ptr(steps), ntones, window)

    for args in ((4, ok, 0, 500), (4, ok, 65, 500), (4, ok, 2, 15), (4, ok, 2, 65537), (0, ok, 2, 500),
                 (4, np.array([5, 0], np.uint32), 2, 500), (4, np.array([5, 1 << 31], np.uint32), 2, 500)):
        assert create(*args) == capi.WR_ERR_ARG, args[0:1] + args[2:]
        assert b"wr_tones_create" in lib.wr_last_error()
    bank = _bank(dev, 2, ok[:2], 16)
    p = dev.upload(np.zeros(64, np.float32))
    try:
        assert lib.wr_tones_push_rows(bank.h, C.c_void_p(p), 16, 3, 16) == capi.WR_ERR_ARG     # nrows > max_rows
        assert lib.wr_tones_push_rows(bank.h, C.c_void_p(p), 15, 2, 16) == capi.WR_ERR_ARG     # rows that overlap
        assert lib.wr_tones_push_rows(bank.h, None, 16, 2, 16) == capi.WR_ERR_ARG
        assert lib.wr_tones_read(bank.h, None, None, None, None, None) == capi.WR_ERR_ARG
        assert lib.wr_tones_reset(bank.h, 2) == capi.WR_ERR_ARG
        assert lib.wr_tones_push_rows(bank.h, C.c_void_p(p), 15, 1, 16) == capi.WR_OK          # one row: any stride
        assert list(bank.read()[2]) == [1, 0]
    finally:
        bank.destroy()
        dev.free(p)
