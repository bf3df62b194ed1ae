"""The voice bank's rule (include/webradio_amd.h: VOICE BANK) restated in float32 numpy -- what the GPU tests compare bits
with.  test_voice_capi.py holds it to the rule written as plain loops (LoopBank below) and to an ideal delayed sine.

    x'   = 0 for an inf or a NaN, else min(max(x, -65536), 65536)                          (resamp_np.clean)
    acc = +0;  for k = 0 .. T-1:  acc = acc + c[f][k] * x'[n - k];  y[n] = mute ? +0 : acc (float32, one rounding each)

A row's control word: bits 0-7 the filter f, bit 8 mute.  Bank keeps, as the rule says, the last T - 1 cleaned inputs of
every row; LoopBank keeps the whole stream of ONE row."""
import numpy as np

from resamp_np import clean

F32 = np.float32
MUTE = 0x100
GRID = 32768
BETA = 6.0


def half_width(audio_rate, T):
    """W: the transition half-width on each side of an edge, Hz"""
    return (BETA / 0.1102 + 8.7 - 8.0) / (2.285 * 2.0 * np.pi * (T - 1)) * audio_rate


def desired(audio_rate, f, highpass_hz, lowpass_hz, deemph_us):
    """D at the frequencies f (float64, Hz)"""
    band = np.ones(f.shape, bool)
    if highpass_hz:
        band &= f >= highpass_hz
    if lowpass_hz:
        band &= f <= lowpass_hz
    de = np.ones(f.shape)
    if deemph_us:
        tau = deemph_us * 1e-6
        de = np.sqrt((1.0 + (2.0 * np.pi * 1000.0 * tau) ** 2) / (1.0 + (2.0 * np.pi * f * tau) ** 2))
    return band * de


def design(audio_rate, T, highpass_hz=300, lowpass_hz=3000, deemph_us=0):
    """float32 [T]: the header's frequency-sampled filter under a Kaiser window, in float64, rounded to float32 once"""
    N, d = T - 1, T // 2 - 1
    f = np.arange(GRID // 2 + 1, dtype=np.float64) * audio_rate / GRID
    h = np.fft.irfft(desired(audio_rate, f, highpass_hz, lowpass_hz, deemph_us), GRID)    # h[n]: the response at lag n, even
    taps = np.zeros(T, np.float32)
    taps[:N] = (h[(np.arange(N) - d) % GRID] * np.kaiser(N, BETA)).astype(np.float32)
    return taps


class Bank:
    """max_rows streams; push(x[nrows][n]) -> y[nrows][n], vectorised over rows and frames, a loop over k"""

    def __init__(self, max_rows, taps):
        self.taps = np.atleast_2d(np.ascontiguousarray(taps, dtype=np.float32))
        self.F, self.T = self.taps.shape
        self.hist = np.zeros((max_rows, self.T - 1), np.float32)
        self.ctl = np.zeros(max_rows, np.uint32)
        self.frames = 0

    def set_rows(self, first, words):
        words = np.asarray(words, np.uint32).reshape(-1)
        assert not np.any(words & ~np.uint32(0x1FF)) and np.all((words & 0xFF) < self.F)
        self.ctl[first: first + words.size] = words

    def reset(self, row=-1):
        if row < 0:
            self.hist[:] = 0
            self.frames = 0
        else:
            self.hist[row] = 0

    def push(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        nrows, n = x.shape
        H = self.T - 1
        ext = np.concatenate([self.hist[:nrows], clean(x)], axis=1)         # ext[:, H + i] is frame i of the push
        c = self.taps[self.ctl[:nrows] & 0xFF]                              # [nrows][T]
        y = np.zeros((nrows, n), np.float32)
        for k in range(self.T):
            y = y + c[:, k][:, None] * ext[:, H - k: H - k + n]
        y[(self.ctl[:nrows] & MUTE) != 0] = F32(0.0)
        if n:
            self.hist[:nrows] = ext[:, ext.shape[1] - H:]
            self.hist[nrows:] = 0                                           # the rows a push leaves out saw nothing
        self.frames += n
        return y


class LoopBank:
    """ONE row, the rule's lines one output and one tap at a time, on the whole stream since its last reset"""

    def __init__(self, taps):
        self.taps = np.atleast_2d(np.ascontiguousarray(taps, dtype=np.float32))
        self.x = []                                                         # cleaned frames
        self.word = 0

    def reset_row(self):
        self.x = []

    def push(self, x):
        f, mute = self.word & 0xFF, bool(self.word & MUTE)
        out = []
        for v in np.asarray(x, dtype=np.float32).reshape(-1):
            bits = int(np.array([v], np.float32).view(np.uint32)[0])
            if (bits & 0x7FFFFFFF) >= 0x7F800000:
                v = F32(0.0)
            self.x.append(F32(min(max(v, F32(-65536.0)), F32(65536.0))))
            n = len(self.x) - 1
            acc = F32(0.0)
            for k in range(self.taps.shape[1]):
                xv = self.x[n - k] if n - k >= 0 else F32(0.0)
                acc = F32(acc + F32(self.taps[f, k] * xv))
            out.append(F32(0.0) if mute else acc)
        return np.array(out, np.float32)
