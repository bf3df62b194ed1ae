"""Case builders the GPU tests of the per-row features share (test_gpu_tones, test_gpu_resamp, test_gpu_voice, test_gpu_agc,
test_gpu_chan_levels, test_gpu_scripts, test_gpu_bank_limits): rows of audio with every awkward float among them, rows in
device memory -- the layout rule by row count, the push into a sentinel-padded output and its comparison -- and
sentinel-filled outputs, the five-receiver NFM tuner of tones_np with its twelve blocks (the fm_stream fixture), the audio of
its untouched twin and a raw wr_tuner_*_push into sentinel-filled rows, and the keyed-carrier block of the level and AGC tests.

Everything random comes from a seeded numpy Generator through a fixed sequence of calls, so a case is the same floats
wherever and whenever it is built."""
import ctypes as C

import numpy as np
import pytest

import tones_np
from capicases import same_bits  # noqa: F401  (bit-for-bit equality of float32 arrays, as rowcases.same_bits too)
from webradio_amd import capi
from webradio_amd.device import Tuner


# ---- plain rows -----------------------------------------------------------------------------------------------------------------

# the awkward floats of the resampler's and the bank-limit tests' rows: non-finite, saturating, signed zero, subnormal, 2^16
SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, -0.0, 1e-40, 65536.0]


def special_rows(nrows, n, seed, max_exp, special):
    """[nrows][n] float32: normal deviates times 10^e, e in [-4, max_exp), both signs, and in every row the values of
    `special` (non-finite, saturating, signed-zero, subnormal ...) at places of its own"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((nrows, n)) * 10.0 ** rng.integers(-4, max_exp, (nrows, n))).astype(np.float32)
    for r in range(nrows):
        where = rng.choice(n, size=min(n, len(special)), replace=False)
        for k, at in enumerate(where):
            v[r, at] = np.float32(special[k])
    return v


# ---- rows in device memory ------------------------------------------------------------------------------------------------------

SENTINEL = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]          # a NaN nobody computes: what a kernel leaves alone


def row_layout(nrows, n):
    """(extra, lead) for rows of n floats: one row back to back; three rows an odd stride and a base one float off 16-byte
    alignment; 64 rows a stride that is a multiple of four and larger than the row; 65 rows odd again"""
    extra, lead = {1: (0, 0), 3: (5, 1), 64: (8 - n % 4, 0), 65: (7, 1)}.get(nrows, (3, 1))
    if (n + extra) % 2 == 0 and nrows in (3, 65):
        extra += 1
    return extra, lead


def upload_laid_out(dev, v):
    """the rows in device memory behind `lead` floats, `stride` floats apart (row_layout), the gaps NaN -- they are never
    read: (pointer to free, pointer to row 0, stride)"""
    nrows, n = v.shape
    extra, lead = row_layout(nrows, n)
    stride = n + extra
    buf = np.full(lead + nrows * stride, np.float32(np.nan), np.float32)
    for r in range(nrows):
        buf[lead + r * stride: lead + r * stride + n] = v[r]
    p = dev.upload(buf)
    return p, p + 4 * lead, stride


def padded_push(dev, nrows, n_out, push, what):
    """`push(p_out, out_stride)` writes nrows rows of n_out floats into a buffer laid out by row_layout and filled with
    SENTINEL: (what push returned, check) -- check(ref) holds every output bit to ref[nrows][n_out], then that nothing
    beside the rows was written"""
    extra, lead = row_layout(nrows, max(n_out, 1))
    ostride = n_out + extra
    obuf = np.full(lead + nrows * ostride + 3, SENTINEL, np.float32)
    p_out = dev.upload(obuf)
    try:
        result = push(p_out + 4 * lead, ostride)
        got = dev.download(p_out, obuf.size)
    finally:
        dev.free(p_out)

    def check(ref):
        out = got[lead: lead + nrows * ostride].reshape(nrows, ostride)
        bad = np.argwhere(out[:, :n_out].view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, (what, len(bad), bad[:4], [out[tuple(b)] for b in bad[:4]], [ref[tuple(b)] for b in bad[:4]])
        gaps = np.concatenate([got[:lead], out[:, n_out:].reshape(-1), got[lead + nrows * ostride:]])
        assert np.all(gaps.view(np.uint32) == SENTINEL.view(np.uint32)), what

    return result, check


def upload_rows(dev, v, stride):
    """the rows `stride` floats apart in device memory, NaN between them: the pointer (the caller frees it)"""
    nrows, n = v.shape
    buf = np.full((nrows, stride), np.float32(np.nan), np.float32)
    buf[:, :n] = v
    return dev.upload(buf)


class OutRows:
    """nrows rows of `stride` floats in device memory for what a push writes, filled with SENTINEL.  peek(rows, frames)
    downloads them and checks that nothing but the first `frames` floats of the first `rows` rows was written; arm() fills
    them again (an upload waits for the device's stream, and so closes an open streaming launch: a caller who wants the push
    itself to do that arms behind the push, not in front of it); take() is both."""

    def __init__(self, dev, nrows, stride):
        self.dev, self.nrows, self.stride = dev, nrows, stride
        self.fill = np.full(nrows * stride, SENTINEL, np.float32)
        self.p = dev.upload(self.fill)

    def arm(self):
        capi.check(self.dev.lib.wr_dev_upload(self.dev.h, self.p, capi.ptr(self.fill), self.fill.nbytes))

    def peek(self, nrows, nframes, what=None):
        assert nrows <= self.nrows and nframes <= self.stride, (what, nrows, nframes)
        got = self.dev.download(self.p, self.fill.size).reshape(self.nrows, self.stride)
        for gap in (got[:nrows, nframes:], got[nrows:]):
            assert np.all(gap.view(np.uint32) == SENTINEL.view(np.uint32)), what
        return got[:nrows, :nframes].copy()

    def take(self, nrows, nframes, what=None):
        got = self.peek(nrows, nframes, what)
        self.arm()
        return got

    def free(self):
        self.dev.free(self.p)


def dcs_bank(dev, max_rows, words, step, max_errors=0):
    """a device.DcsBank on a caller's step: its constructor takes an audio rate and asks wr_dcs_step, which refuses rates
    below two frames per chip; wr_dcs_create itself takes any step in [2^19, 2^28]"""
    from webradio_amd.device import DcsBank
    b = DcsBank.__new__(DcsBank)
    b.dev, b.lib, b.max_rows, b.step, b.max_errors = dev, dev.lib, max_rows, int(step), max_errors
    b.words = np.array(words, dtype=np.uint32)
    b.ncodes = b.words.size
    h = C.c_void_p()
    capi.check(dev.lib.wr_dcs_create(C.byref(h), dev.h, max_rows, capi.ptr(b.words), b.ncodes, b.step, max_errors))
    b.h = h
    return b


# ---- the five NFM receivers of tones_np behind a tuner --------------------------------------------------------------------------

NBLOCKS, BLOCK = 12, 100_000
K2 = BLOCK // (tones_np.FS // tones_np.AUDIO_RATE)
_twin_audio = {}


def fm_upload(dev):
    """the twelve blocks in device memory, back to back (the caller frees them, and calls forget_twins)"""
    return dev.upload(np.concatenate([tones_np.fm_block(BLOCK, b * BLOCK) for b in range(NBLOCKS)]))


@pytest.fixture(scope="module")
def fm_stream(dev):
    """the twelve blocks in device memory, back to back; uploaded once (a module that uses it imports it)"""
    p = fm_upload(dev)
    yield p
    forget_twins()
    dev.free(p)


def raw_tuner_push(dev, call, stride, out=True):
    """a wr_tuner_*_push that writes rows: `call(out_dev, out_stride)` -> rc with a buffer of 64 rows of `stride` floats
    filled with SENTINEL (out False: a NULL out_dev); (rc, the rows downloaded)"""
    p = dev.upload(np.full(64 * stride, SENTINEL, np.float32))
    try:
        rc = call(C.c_void_p(p) if out else None, stride)
        got = dev.download(p, 64 * stride).reshape(64, stride)
    finally:
        dev.free(p)
    return rc, got


def fm_tuner(dev, nco, streaming=False, spare=0):
    t = Tuner(dev, tones_np.FS, len(tones_np.IFS) + spare, BLOCK, nco)
    chans = [t.add_receiver(f, tones_np.CHAN_PASSBAND, tones_np.CHAN_RATE, capi.WR_FM, tones_np.AUDIO_PASSBAND,
                            tones_np.AUDIO_RATE) for f in tones_np.IFS]
    if streaming:
        t.streaming(True)
    return t, chans


def twin_audio(dev, x, nco, streaming=False):
    """[block][receiver] audio of the same tuner that never sees the call under test, a fetch per block; run once per NCO
    mode and way of launching"""
    key = (nco, streaming)
    if key not in _twin_audio:
        _twin_audio[key] = block_audio(fm_tuner(dev, nco, streaming), x, NBLOCKS, BLOCK, K2)
    return _twin_audio[key]


def block_audio(tuner, x, nblocks, block, k2):
    """[block][receiver] audio of `tuner` = (tuner, channels) over `nblocks` blocks of `block` frames at x, a launch and a fetch
    per block; the tuner is destroyed"""
    t, chans = tuner
    out = []
    for b in range(nblocks):
        t.submit_device(x + 8 * block * b, block)
        out.append([t.fetch(ch, capi.WR_STAGE_AUDIO, k2) for ch in chans])
    t.destroy()
    return out


def forget_twins():
    _twin_audio.clear()


# ---- a block of keyed carriers --------------------------------------------------------------------------------------------------

def channel_ifs(nrx):
    return [(c - nrx // 2) * 25_000 + 321 for c in range(nrx)]


def keyed_block(nframes, ifs, seed, pos=0, scale=1.0, fs=2_000_000):
    """noise in every channel, and a carrier keyed at 150 Hz on each of `ifs`"""
    tt = (np.arange(nframes) + pos) / fs
    iq = (0.002 * scale * np.random.default_rng(seed).standard_normal(2 * nframes)).astype(np.float32)
    env = 0.02 * scale * (1.0 + np.sign(np.sin(2 * np.pi * 150.0 * tt))) * 0.5
    for f in ifs:
        ph = 2 * np.pi * ((f * tt) % 1.0)
        iq[0::2] += (env * np.cos(ph)).astype(np.float32)
        iq[1::2] += (env * np.sin(ph)).astype(np.float32)
    return iq
