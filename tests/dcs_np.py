"""The DCS bank's rule (include/webradio_amd.h: DCS BANK) restated in vectorised numpy -- what the GPU tests compare bits with.
The clock is a Python integer, so N * step beyond 2^64 is exact here; everything per frame is an array operation.

    word(code):  d = code | 0x800;  p = d;  twelve times: if p & 1: p ^= 0xC75;  p >>= 1;   word = (p << 12) | d
    step_of(rate) = (672 * 2^32 + (5 rate) // 2) // (5 rate)                     134.4 Hz in units of 2^-32 bit per frame
    frame n belongs to chip g(n) = (n * step) >> 29;   C[g] += (int64)rint(clamp(v', -64, 64) * 2^24)
    evaluation e (once g(N) >= 8 e), phase f = 0 .. 7:  B_b = sum_{c < 8} C[8 e - 184 - f + 8 b + c],  b = 0 .. 22
    w_f = sum_b 2^b [2 B_b > max B + min B];   agree[k] = max over f and the 23 rotations of (23 - popcount, popcount)

Besides the Bank: the test signals (signal_row: NRZ of a word under a 400 Hz "voice" tone, DC and noise) and the tuner case
(fm_block: six FM carriers that carry such signals as frequency deviation)."""
import numpy as np
from scipy.signal import lfilter

STEP_MIN, STEP_MAX = 1 << 19, 1 << 28
HIST = 192                                              # chips kept in front of the open one: an evaluation reaches back 191

_PC16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)


def word(code):
    assert 0 <= code < 512
    d = code | 0x800
    p = d
    for _ in range(12):
        if p & 1:
            p ^= 0xC75
        p >>= 1
    return (p << 12) | d


def step_of(audio_rate):
    """None where the C ABI refuses the rate"""
    if audio_rate <= 0:
        return None
    step = (672 * (1 << 32) + (5 * audio_rate) // 2) // (5 * audio_rate)
    return step if STEP_MIN <= step <= STEP_MAX else None


def rotations(w):
    """the 23 rotations of a 23-bit word"""
    return [((w << r) | (w >> (23 - r))) & 0x7FFFFF for r in range(23)]


def popcount(v):
    v = np.asarray(v, np.uint32)
    return _PC16[v & np.uint32(0xFFFF)] + _PC16[v >> np.uint32(16)]


def quantise(v):
    """q (int64): an inf or a NaN counts as 0, the rest is clamped to +-64 and scaled by 2^24 (the tone bank's cleaning)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    bad = (v.view(np.uint32) & np.uint32(0x7FFFFFFF)) >= np.uint32(0x7F800000)
    c = np.minimum(np.maximum(np.where(bad, np.float32(0.0), v), np.float32(-64.0)), np.float32(64.0))
    return np.rint(c * np.float32(16777216.0)).astype(np.int64)


# B_b of phase f is cs[s + 8] - cs[s] with s = 7 - f + 8 b, cs the running sum of chips 8 e - 191 ... 8 e - 1
_S = (7 - np.arange(8)[:, None] + 8 * np.arange(23)[None, :]).astype(np.int64)


def received_words(chips):
    """w[..., 8] (uint32) of evaluations whose 191 chips 8 e - 191 ... 8 e - 1 are chips[..., 191]"""
    chips = np.asarray(chips, np.int64)
    assert chips.shape[-1] == 191
    cs = np.concatenate([np.zeros(chips.shape[:-1] + (1,), np.int64), np.cumsum(chips, axis=-1)], axis=-1)
    B = cs[..., _S + 8] - cs[..., _S]                                     # [..., 8][23]
    thr = B.max(axis=-1, keepdims=True) + B.min(axis=-1, keepdims=True)
    bits = (2 * B > thr).astype(np.uint32)
    return (bits << np.arange(23, dtype=np.uint32)).sum(axis=-1, dtype=np.uint32)


class Bank:
    """max_rows streams on ONE clock; push(x[nrows][n]) continues rows 0 .. nrows-1 and resets the rows it leaves out"""

    def __init__(self, max_rows, words, step, max_errors=0):
        self.words = [int(w) for w in words]
        assert 1 <= len(self.words) <= 128 and all(0 <= w < 1 << 23 for w in self.words)
        assert STEP_MIN <= step <= STEP_MAX and 0 <= max_errors <= 3
        self.max_rows, self.step, self.max_errors = max_rows, int(step), int(max_errors)
        self.rots = np.array([rotations(w) for w in self.words], np.uint32)           # [ncodes][23]
        n = len(self.words)
        self.agree = np.zeros((max_rows, n, 2), np.uint8)
        self.run = np.zeros((max_rows, n, 2), np.uint32)
        self.hits = np.zeros((max_rows, n, 2), np.uint64)
        self.evals = np.zeros(max_rows, np.uint64)
        self.seek(0)

    def _chip(self, frame):
        return (frame * self.step) >> 29

    def seek(self, frame):
        self.N = int(frame)
        self.base = self._chip(self.N) - HIST                                         # chips[:, i] is chip base + i
        self.chips = np.zeros((self.max_rows, HIST + 1), np.int64)
        for a in (self.agree, self.run, self.hits, self.evals):
            a[...] = 0

    def reset(self, row=-1):
        if row < 0:
            self.seek(0)
        else:
            self._zero(slice(row, row + 1))

    def _zero(self, rows):
        for a in (self.chips, self.agree, self.run, self.hits, self.evals):
            a[rows] = 0

    def push(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        nrows, n = x.shape
        assert nrows <= self.max_rows and n <= 1 << 28
        if not n:
            return
        self._zero(slice(nrows, None))
        a0 = self.N * self.step
        g0, ph0 = a0 >> 29, a0 & ((1 << 29) - 1)
        g1 = self._chip(self.N + n)
        grow = g1 - self.base + 1 - self.chips.shape[1]
        if grow > 0:
            self.chips = np.concatenate([self.chips, np.zeros((self.max_rows, grow), np.int64)], axis=1)
        if nrows:
            off = (np.uint64(ph0) + np.arange(n, dtype=np.uint64) * np.uint64(self.step)) >> np.uint64(29)
            starts = np.flatnonzero(np.diff(off.astype(np.int64), prepend=-1))        # every chip from g0 on holds a frame
            lo = g0 - self.base
            self.chips[:nrows, lo: lo + starts.size] += np.add.reduceat(quantise(x), starts, axis=1)
        first, last = g0 // 8 + 1, g1 // 8                                            # the evaluations of this push
        room = max(1, (1 << 22) // max(1, nrows * 8 * len(self.words) * 23))
        for e0 in range(first, last + 1, room):
            es = np.arange(e0, min(e0 + room, last + 1))
            col = (8 * es - 191 - self.base)[:, None] + np.arange(191)[None, :]
            self._evaluate(nrows, received_words(self.chips[:nrows][:, col]))
        self.N += n
        keep = self._chip(self.N) - HIST
        self.chips = np.ascontiguousarray(self.chips[:, keep - self.base:])
        self.base = keep

    def _evaluate(self, nrows, w):
        """w[nrows][E][8]: E consecutive evaluations"""
        x = popcount(w[:, :, :, None, None] ^ self.rots[None, None, None, :, :])      # [rows][E][8][ncodes][23]
        most, least = x.max(axis=(2, 4)), x.min(axis=(2, 4))                           # [rows][E][ncodes]
        agree = np.stack([23 - least, most], axis=-1).astype(np.uint8)                 # [rows][E][ncodes][2]
        match = agree >= 23 - self.max_errors
        for e in range(w.shape[1]):
            m = match[:, e]
            self.hits[:nrows] += m.astype(np.uint64)
            self.run[:nrows] = np.where(m, self.run[:nrows] + np.uint32(1), np.uint32(0))
        if w.shape[1]:
            self.agree[:nrows] = agree[:, -1]
            self.evals[:nrows] += np.uint64(w.shape[1])

    def read(self):
        return self.agree, self.run, self.hits, self.evals


# ---- signals --------------------------------------------------------------------------------------------------------------------

BIT_HZ = 134.4
VOICE_HZ = 400.0


def nrz(w, rate, n, pos=0, start=0.0, inverted=False, smooth_hz=300.0):
    """frames [pos, pos + n) of the word sent over and over, bit 0 first, as +-1 NRZ (a set bit is +1; `inverted`: -1)
    through a one-pole smoother with its corner at smooth_hz; `start`: the bit position (fractional) of frame 0.  Every
    call computes the stream from frame 0, so any cut gives the same floats."""
    t = np.arange(pos + n, dtype=np.float64)
    bit = np.floor(t * (BIT_HZ / rate) + start).astype(np.int64) % 23
    level = np.where((int(w) >> bit) & 1, 1.0, -1.0) * (-1.0 if inverted else 1.0)
    a = 1.0 - np.exp(-2.0 * np.pi * smooth_hz / rate)
    return lfilter([a], [1.0, a - 1.0], level)[pos:]


def signal_row(w, rate, n, seed, amp=0.05, start=0.0, inverted=False, dc=0.25, noise=0.01):
    """float32 [n]: the NRZ of `w` (None: no code) at amplitude amp, a 400 Hz tone of twice that, DC and seeded noise"""
    t = np.arange(n, dtype=np.float64) / rate
    v = dc + 2.0 * amp * np.sin(2.0 * np.pi * VOICE_HZ * t + 0.7)
    if w is not None:
        v = v + amp * nrz(w, rate, n, 0, start, inverted)
    return (v + noise * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ---- the tuner test's case: six NFM receivers; four carry a code (one inverted), one voice only, one a bare carrier --------------

FS, CHAN_RATE, AUDIO_RATE = 2_000_000, 20_000, 5_000
CHAN_PASSBAND, AUDIO_PASSBAND = 128_000, 2_500
BLOCK, NBLOCKS = 100_000, 10
K2 = BLOCK // (FS // AUDIO_RATE)
IFS = (-750_321, -450_123, -150_077, 150_211, 450_433, 750_119)
CODED = ((0o023, False, 0.0), (0o754, True, 3.3), (0o412, False, 11.71), (0o131, False, 20.5))   # (code, inverted, start bit)
CARRIER, DCS_DEV, VOICE_DEV, NOISE = 0.12, 700.0, 1_400.0, 0.001
AUDIO_SIGN = -1.0            # the chain's FM discriminator output FALLS as the frequency rises: CODED's polarity is the audio's
_stream = None


def fm_stream():
    """interleaved float32 IQ of the whole stream, NBLOCKS * BLOCK frames: receivers 0 .. 3 carry CODED and the voice tone,
    receiver 4 the voice tone alone, receiver 5 is a bare carrier; built once"""
    global _stream
    if _stream is None:
        n = NBLOCKS * BLOCK
        t = np.arange(n, dtype=np.float64) / FS
        voice = VOICE_DEV * np.sin(2.0 * np.pi * VOICE_HZ * t)
        z = np.zeros(n, np.complex128)
        for r, f in enumerate(IFS):
            hz = np.zeros(n) if r == 5 else voice.copy()
            if r < len(CODED):
                code, inverted, start = CODED[r]
                hz += AUDIO_SIGN * DCS_DEV * nrz(word(code), FS, n, 0, start, inverted)
            ph = 2.0 * np.pi * (((f * t) % 1.0) + np.cumsum(hz) / FS)
            z += CARRIER * np.exp(1j * ph)
        rng = np.random.default_rng(23)
        z += NOISE * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        out = np.empty(2 * n, np.float32)
        out[0::2], out[1::2] = z.real, z.imag
        _stream = out
    return _stream


def fm_block(b):
    return fm_stream()[2 * BLOCK * b: 2 * BLOCK * (b + 1)]


def partner(words, own):
    """indices of the words of `words` that are a rotation of the complement of words[own]: its inverse partner"""
    inv = set(rotations(~words[own] & 0x7FFFFF))
    return [k for k, w in enumerate(words) if w in inv]


def detection(agree, run, words, rows):
    """the detection conditions at the end of the tuner case's stream, on agree / run [6 receivers][ncodes][2] of `rows`;
    `words` are the standard codes' in DCS_CODES' order.  Returns (own runs, largest foreign run) for printing."""
    from webradio_amd import DCS_CODES
    own_runs, foreign = [], 0
    for r, row in enumerate(rows):
        allowed = set()
        if r < len(CODED):
            code, inverted, _ = CODED[r]
            own = DCS_CODES.index(code)
            pol = 1 if inverted else 0
            assert int(agree[row, own, pol]) == 23, (r, int(agree[row, own, pol]))
            assert int(run[row, own, pol]) >= 8, (r, int(run[row, own, pol]))
            own_runs.append(int(run[row, own, pol]))
            allowed = {(own, pol)} | {(k, 1 - pol) for k in partner(words, own)}
        for k in range(len(words)):
            for pol in (0, 1):
                if (k, pol) not in allowed:
                    foreign = max(foreign, int(run[row, k, pol]))
                    assert int(run[row, k, pol]) < 2, (r, oct(DCS_CODES[k]), pol, int(run[row, k, pol]))
    return own_runs, foreign
