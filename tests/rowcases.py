"""Case builders the GPU tests of the per-row features share (test_gpu_tones, test_gpu_resamp, test_gpu_agc,
test_gpu_chan_levels, test_gpu_scripts, test_gpu_bank_limits): rows of audio with every awkward float among them, rows in
device memory and sentinel-filled outputs, the five-receiver NFM tuner of tones_np with its twelve blocks and the audio of
its untouched twin, and the keyed-carrier block of the level and AGC tests.

Everything random comes from a seeded numpy Generator through a fixed sequence of calls, so a case is the same floats
wherever and whenever it is built."""
import numpy as np

import tones_np
from webradio_amd import capi
from webradio_amd.device import Tuner


# ---- plain rows -----------------------------------------------------------------------------------------------------------------

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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


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
    import ctypes as C
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
        t, chans = fm_tuner(dev, nco, streaming)
        out = []
        for b in range(NBLOCKS):
            t.submit_device(x + 8 * BLOCK * b, BLOCK)
            out.append([t.fetch(ch, capi.WR_STAGE_AUDIO, K2) for ch in chans])
        t.destroy()
        _twin_audio[key] = out
    return _twin_audio[key]


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
