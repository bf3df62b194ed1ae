"""The flat input of the all-bins spectrum tests and what they measure against oracle.spectrum_np.

White noise: every bin has comparable power, so the mask the spectrum tests put on dB values -- bins within 60 dB of the
frame's peak -- keeps essentially every bin (tests/test_spectrum_flat_reference.py asserts how many it leaves out) where
the carriers of synth.fm_stream leave it 0.1 ... 70 % of them.  Samples are integers in [-2^14, 2^14) times 2^-15 from a
seeded Generator: exact in float32 and the same bits on every host (tests/refcases.py uses the same grid)."""
import numpy as np

import wr_oracle

MASK_DB = 60.0                  # the spectrum tests' mask: dB is compared on bins within this of the frame's peak
MASK_OUT_SHARE = 1e-3           # at most this share of a frame's bins may lie outside it


def flat(count, seed):
    """`count` float32 samples: IQ interleaved (count = 2 * frames) or one channel"""
    q = np.random.default_rng(seed).integers(-(1 << 14), 1 << 14, count)
    return q.astype(np.float32) / np.float32(1 << 15)


def frames_of(stream, n, hop, real=False):
    """a view (frames, n) of every whole frame of a stream, frames `hop` apart: complex64, or float32 if real"""
    v = stream if real else stream.view(np.complex64)
    return np.lib.stride_tricks.sliding_window_view(v, n)[::hop]


def interleaved(bins):
    out = np.empty(bins.shape[:-1] + (2 * bins.shape[-1],), np.float64)
    out[..., 0::2], out[..., 1::2] = bins.real, bins.imag
    return out


def left_out(want_db):
    """per frame: how many bins the mask leaves out"""
    want_db = np.atleast_2d(want_db)
    return (want_db < want_db.max(axis=-1, keepdims=True) - MASK_DB).sum(axis=-1)


def bin_error(got_bins, want_bins):
    """max |got - want| over all bins of one frame as a multiple of the frame's peak bin; `got_bins` interleaved float32.
    NaN if anything in `got_bins` is."""
    return float(np.abs(got_bins.astype(np.float64) - interleaved(want_bins)).max() / np.abs(want_bins).max())


def db_error(got_db, want_db):
    """(max |got - want| in dB over the masked bins of every frame, most bins the mask leaves out of one frame)"""
    got_db, want_db = np.atleast_2d(got_db), np.atleast_2d(want_db)
    strong = want_db >= want_db.max(axis=-1, keepdims=True) - MASK_DB
    return float(np.abs(got_db - want_db)[strong].max()), int((~strong).sum(axis=-1).max())


def rows_db_error(got, stream, n, hop, frames, real=False, points=1 << 21):
    """db_error of the dB rows `got` (frames, n) against oracle.spectrum_np of every frame of `stream`, every bin; the
    reference is computed `points` points at a time"""
    view = frames_of(stream, n, hop, real)
    assert view.shape[0] >= frames and got.shape == (frames, n)
    step = max(1, points // n)
    err, out = 0.0, 0
    for r in range(0, frames, step):
        want_db = wr_oracle.spectrum_np(np.ascontiguousarray(view[r: min(r + step, frames)]))[0]
        e, o = db_error(got[r: r + want_db.shape[0]], want_db)
        err, out = (e if e > err or e != e else err), max(out, o)
        if err != err:
            break
    return err, out
