"""What the tests of wr_spectrum_batch_avg and wr_spectrum_rows_waterfall share: the shapes, the float32 restatement of the
rule, the float64 reference and the restatement of k_waterfall_row for rows.  No tests here.

The rule (include/webradio_amd.h): for bin k of a group, p_f = fl(fl(re*re) + fl(im*im)) of frame f's bin, sum one float32
accumulator that starts at p_0 and adds p_1, p_2, ... in frame order, mean = sum / float32(F), peak the largest p_f; rows
fft-shifted; dB is 10*log10(x) - 20*log10(n).

The reference: oracle.spectrum_np per frame (float32 window product, float64 FFT, dB), 10**(dB/10), mean or max over the
frames of a group, back to dB -- all in float64."""
import functools

import numpy as np

import wr_oracle
from flat_spectrum import MASK_DB, flat, frames_of

# (n, hop, F) of the every-path test: k_fft_single, the generic four-step, the 65536-point register path with one and with
# four frames per pass-1 workgroup, past the work area's chunk of 256 frames at 65536 points and of 16 at 1048576
IQ_SHAPES = [(8, 3, 300), (512, 128, 70), (8192, 1000, 9), (16384, 4096, 7), (32768, 5000, 5), (65536, 32768, 5),
             (65536, 4096, 97), (65536, 1024, 259), (1048576, 4096, 17)]
REAL_SHAPES = [(16, 16, 40), (16384, 3000, 6), (32768, 5000, 5), (524288, 65536, 3)]
# (real, n, hop, F, groups, group_stride)
GROUP_SHAPES = [(False, 512, 200, 3, 70, 1117),         # one launch for all groups
                (True, 256, 128, 14, 256, 2000),        # the audio block's shape
                (False, 16384, 4096, 2, 3, 16384 + 4096 + 77)]   # the looped two-pass form
# (real, n, hop) of the bit tests, each at F in BIT_FRAMES: the single-workgroup sizes, a hop different from n
BIT_SHAPES = [(False, 8, 5), (False, 512, 200), (False, 8192, 1000), (True, 16, 7), (True, 16384, 3001)]
BIT_FRAMES = (1, 2, 5)

BURST_N, BURST_F, BURST_AT, BURST_BIN = 512, 8, 3, 64


def span(n, hop, F):
    """frames (IQ) or samples (real) that F frames at `hop` cover"""
    return n + (F - 1) * hop


def seed_of(*shape):
    return 4000 + sum(int(v) * (i + 1) for i, v in enumerate(shape))


def stream_of(real, n, hop, F, groups=1, stride=0):
    """the flat input of a shape: float32, interleaved IQ unless `real`"""
    total = span(n, hop, F) + (groups - 1) * stride
    return flat(total if real else 2 * total, seed_of(real, n, hop, F, groups, stride))


def group_frames(stream, real, n, hop, F, g=0, stride=0):
    """the (F, n) frames of group g: complex64, or float32 if real"""
    ch = 1 if real else 2
    part = stream[ch * g * stride: ch * (g * stride + span(n, hop, F))]
    return np.ascontiguousarray(frames_of(part, n, hop, real)[:F])


# ---- the float32 restatement --------------------------------------------------------------------------------------------

def power32(bins):
    """p_f of interleaved float32 bins (..., 2n): two products and one sum, each rounded to float32"""
    bins = np.asarray(bins, np.float32)
    re, im = bins[..., 0::2], bins[..., 1::2]
    return re * re + im * im


def restate_linear(bins):
    """(mean, peak) rows, linear and fft-shifted, of the bins (F, 2n) of one group's frames, in the rule's order"""
    p = power32(bins)
    assert p.dtype == np.float32 and p.ndim == 2
    s = p[0].copy()
    for f in range(1, p.shape[0]):
        s = s + p[f]
    mean = s / np.float32(p.shape[0])
    assert s.dtype == np.float32 and mean.dtype == np.float32
    return np.fft.fftshift(mean), np.fft.fftshift(p.max(axis=0))


def to_db64(x, n):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(x, np.float64)) - 20.0 * np.log10(float(n))


# ---- the float64 reference ------------------------------------------------------------------------------------------------

def reference_db(frames, points=1 << 21):
    """(mean, peak) dB rows in float64 of the frames (F, n) of one group; oracle.spectrum_np `points` points at a time"""
    F, n = frames.shape
    step = max(1, points // n)
    total, top = np.zeros(n), np.zeros(n)
    for r in range(0, F, step):
        lin = 10.0 ** (wr_oracle.spectrum_np(np.ascontiguousarray(frames[r: r + step]))[0] / 10.0)
        total += lin.sum(axis=0)
        top = np.maximum(top, lin.max(axis=0))
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(total / F), 10.0 * np.log10(top)


@functools.lru_cache(maxsize=None)
def reference_of(real, n, hop, F, groups=1, stride=0):
    """(stream, mean rows, peak rows) of a shape's flat input, rows (groups, n) float64: computed once per session"""
    stream = stream_of(real, n, hop, F, groups, stride)
    rows = [reference_db(group_frames(stream, real, n, hop, F, g, stride)) for g in range(groups)]
    mean, peak = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    for a in (stream, mean, peak):
        a.setflags(write=False)
    return stream, mean, peak


def masked_error(got, want):
    """(max |got - want| in dB on the bins within MASK_DB of their row's peak, most bins the mask leaves out of one row)"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    strong = want >= want.max(axis=-1, keepdims=True) - MASK_DB
    return float(np.abs(got - want)[strong].max()), int((~strong).sum(axis=-1).max())


# ---- the burst ------------------------------------------------------------------------------------------------------------

def burst_stream():
    """BURST_F back-to-back frames of BURST_N points: a carrier on the centre of bin BURST_BIN in frame BURST_AT only,
    noise 50 dB below it in all frames; interleaved float32"""
    n = BURST_N
    noise = flat(2 * n * BURST_F, seed=77).view(np.complex64)
    amp = 0.5
    rms = float(np.sqrt((np.abs(noise) ** 2).mean()))
    z = (noise * np.float32(amp * 10.0 ** (-50.0 / 20.0) / rms)).astype(np.complex64)
    t = np.arange(n)
    z[BURST_AT * n: (BURST_AT + 1) * n] += (amp * np.exp(2j * np.pi * BURST_BIN * t / n)).astype(np.complex64)
    return np.ascontiguousarray(z).view(np.float32)


BURST_COLUMN = BURST_BIN + BURST_N // 2         # the carrier's place in a shifted row


# ---- k_waterfall_row on rows ----------------------------------------------------------------------------------------------

def rows_waterfall(db_rows, width, hold):
    """(dB per pixel column float32 (rows, width), palette uint8) of shifted float32 dB rows (rows, n): the last of the
    n / width bins of a column or, `hold`, their maximum; non-finite becomes -10000; the palette in double"""
    db_rows = np.atleast_2d(np.asarray(db_rows, np.float32))
    rows, n = db_rows.shape
    d = np.where(np.isfinite(db_rows), db_rows, np.float32(-10000.0)).reshape(rows, width, n // width)
    v = d.max(axis=-1) if hold else d[..., -1]
    pal = np.clip(np.floor((v.astype(np.float64) + 50.0) / 25.0 * 255.0), 0.0, 255.0).astype(np.uint8)
    return v.astype(np.float32), pal
