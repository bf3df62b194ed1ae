"""-m gpu: every row bank at the row limit the header documents, max_rows = 65535 -- for the three kernels that put the row on
blockIdx.y (k_tones_part, k_resamp_rows, k_voice_rows) exactly the grid's limit, for the two that put it on blockIdx.x
(k_dcs_push, k_tones_latch) a grid of that many workgroups -- and row addresses of 65534 strides.

Each bank takes 65535 rows of 40 frames, then of 17, then 65534 rows of 17: the last row is left out, and it is reset where
the bank's convention says so (resampler, DCS bank, voice bank; not the tone bank); the resampler and the voice bank then
take all rows once more, which shows the last row's empty history.  Every row is compared bit for bit with the restatement.
The banks are small -- four and eight taps, one code, two tones -- so that the restatements stay fast.  The rows are 65535
distinct random ones, the awkward floats in the first and the last; the tone bank's repeat with period 97, because
tones_np.Bank walks rows in Python: it computes 97 rows, and row r is compared with row r % 97."""
import numpy as np
import pytest

import dcs_np
import resamp_np
import rowcases
import tones_np
import voice_np
from rowcases import SPECIAL
from webradio_amd.device import Resampler, ToneBank, VoiceBank

pytestmark = pytest.mark.gpu

ROWS, LONG, SHORT, STRIDE = 65535, 40, 17, 40 + 3
PERIOD = 97


@pytest.fixture(scope="module")
def rows():
    """[ROWS][LONG + SHORT] float32, made once and never written: normal deviates times 10^e, e in [-4, 2), the SPECIAL values
    in the first and the last row"""
    rng = np.random.default_rng(65535)
    v = (rng.standard_normal((ROWS, LONG + SHORT)) * 10.0 ** rng.integers(-4, 2, (ROWS, LONG + SHORT))).astype(np.float32)
    for r in (0, ROWS - 1):
        for at in (3, LONG + 2):                                          # in the push of 40 and in the push of 17
            v[r, at: at + len(SPECIAL)] = np.array(SPECIAL, np.float32)
    v.setflags(write=False)
    return v


class _Pushes:
    """the input rows in device memory, STRIDE floats apart, and a sentinel-filled output of the same shape"""

    def __init__(self, dev, v):
        self.dev, self.v = dev, v
        self.p = [rowcases.upload_rows(dev, v[:, :LONG], STRIDE), rowcases.upload_rows(dev, v[:, LONG:], STRIDE)]
        self.out = rowcases.OutRows(dev, ROWS, STRIDE)
        # (which input, rows, frames): all rows of 40 frames, of 17, then all but the last, then all again
        self.plan = [(0, ROWS, LONG), (1, ROWS, SHORT), (0, ROWS - 1, SHORT), (1, ROWS, SHORT)]

    def frames(self, which, nrows, n):
        return (self.v[:, :LONG] if which == 0 else self.v[:, LONG:])[:nrows, :n]

    def close(self):
        for p in self.p:
            self.dev.free(p)
        self.out.free()


def _all_rows_same(got, want, what):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert got.shape == want.shape and bad.size == 0, (what, got.shape, want.shape, len(bad), bad[:4])


def test_resampler_at_the_row_limit(dev, rows):
    """L / M = 3 / 4 with P = 4 and a caller's taps of full size; the fourth push shows the last row's empty history"""
    L, M = resamp_np.ratio(4, 3)
    taps = np.random.default_rng(4).uniform(-16.0, 16.0, (L, 4)).astype(np.float32)
    rs, want, io = Resampler(dev, ROWS, 4, 3, taps=taps), resamp_np.Bank(ROWS, L, M, taps), _Pushes(dev, rows)
    try:
        for which, nrows, n in io.plan:
            n_out = rs.push_rows(io.p[which], STRIDE, nrows, n, io.out.p, STRIDE)
            ref = want.push(io.frames(which, nrows, n))
            assert n_out == ref.shape[1] > 0
            _all_rows_same(io.out.take(nrows, n_out, (nrows, n)), ref, (nrows, n))
        assert rs.info()[3:] == (want.frames_in, want.frames_out)
    finally:
        io.close()
        rs.destroy()


def test_voice_bank_at_the_row_limit(dev, rows):
    """T = 8, two filters, row r on filter r % 2, every 1000th row muted and the last row on filter 1"""
    taps = np.random.default_rng(8).uniform(-16.0, 16.0, (2, 8)).astype(np.float32)
    words = (np.arange(ROWS) % 2).astype(np.uint32)
    words[500::1000] |= VoiceBank.MUTE
    words[ROWS - 1] = 1
    bank, want, io = VoiceBank(dev, ROWS, taps), voice_np.Bank(ROWS, taps), _Pushes(dev, rows)
    try:
        bank.set_rows(0, words)
        want.set_rows(0, words)
        for which, nrows, n in io.plan:
            bank.push_rows(io.p[which], STRIDE, nrows, n, io.out.p, STRIDE)
            _all_rows_same(io.out.take(nrows, n, (nrows, n)), want.push(io.frames(which, nrows, n)), (nrows, n))
        assert bank.info()[2] == want.frames == LONG + 3 * SHORT
    finally:
        io.close()
        bank.destroy()


def test_dcs_bank_at_the_row_limit(dev, rows):
    """one code at the largest step, two frames per chip: three evaluations in the first two pushes, a fourth in the third"""
    words = [dcs_np.word(0o023)]
    bank, want, io = rowcases.dcs_bank(dev, ROWS, words, 1 << 28), dcs_np.Bank(ROWS, words, 1 << 28), _Pushes(dev, rows)
    try:
        for which, nrows, n in io.plan[:3]:
            bank.push_rows(io.p[which], STRIDE, nrows, n)
            want.push(io.frames(which, nrows, n))
        got = bank.read()
        for g, w in zip(got, want.read()):
            assert np.array_equal(g, w)
        assert int(got[3][0]) == int(got[3][ROWS - 2]) == 4 and not any(a[ROWS - 1].any() for a in got)      # the row left out: reset
        assert len({int(a) for a in got[0].reshape(-1)}) > 2              # (the rows do not all say the same)
        assert bank.info()[3] == want.N == LONG + 2 * SHORT
        io.out.peek(0, 0)                                                 # (the bank writes nothing of the kind)
    finally:
        io.close()
        bank.destroy()


def test_tone_bank_at_the_row_limit(dev, rows):
    """two tones, W = 16; row r carries row r % 97 of the input, so the restatement computes 97 rows; the row left out keeps
    what it had after the second push: the tone bank resets nothing"""
    steps = [tones_np.step_of(67.0, 1_000), tones_np.step_of(250.3, 1_000)]
    v = rows[np.arange(ROWS) % PERIOD]
    bank, want, io = ToneBank(dev, ROWS, None, None, 16, steps=steps), tones_np.Bank(PERIOD, steps, 16), _Pushes(dev, v)
    try:
        kept = None
        for at, (which, nrows, n) in enumerate(io.plan[:3]):
            bank.push_rows(io.p[which], STRIDE, nrows, n)
            if at == 2:
                kept = [a[(ROWS - 1) % PERIOD].copy() for a in want.read()]
            want.push(io.frames(which, PERIOD, n))
        for g, w, k in zip(bank.read(), want.read(), kept):
            assert np.array_equal(g[: ROWS - 1], w[np.arange(ROWS - 1) % PERIOD])
            assert np.array_equal(g[ROWS - 1], k)
        assert int(want.windows.min()) == (LONG + 2 * SHORT) // 16 and int(kept[2]) == (LONG + SHORT) // 16
        io.out.peek(0, 0)
    finally:
        io.close()
        bank.destroy()
