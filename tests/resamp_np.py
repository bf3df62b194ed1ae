"""The resampler's rule (include/webradio_amd.h: RESAMPLER) restated in float32 numpy -- what the GPU tests compare bits
with.  test_resamp_capi.py holds it to the rule written as plain loops (LoopBank below) and to an ideal delayed sine.

    x'   = 0 for an inf or a NaN, else min(max(x, -65536), 65536)
    t = m M,  n0 = t // L,  ph = t mod L
    acc = +0;  for k = 0 .. P-1:  acc = acc + c[ph][k] * x'[n0 - k];  y[m] = acc          (float32, one rounding each)

Frame m comes out with the push that holds input frame n0(m).  Bank keeps, as the rule says, only N mod M of the clock;
LoopBank keeps the whole stream and the whole count, so the two are independent in that too."""
import numpy as np

F32 = np.float32
CLAMP = 65536.0


def ratio(in_rate, out_rate):
    g = int(np.gcd(in_rate, out_rate))
    return out_rate // g, in_rate // g


def design(in_rate, out_rate, P):
    """(taps float32 [L][P], L, M): the header's Kaiser-windowed sinc, in float64, rounded to float32 once"""
    L, M = ratio(in_rate, out_rate)
    nh = L * P
    width = 5.0 * in_rate / P
    fc = min(in_rate, out_rate) / 2.0 - width / 2.0
    i = np.arange(nh, dtype=np.float64)
    h = np.sinc(2.0 * fc / (L * in_rate) * (i - (nh - 1) / 2.0)) * np.kaiser(nh, 8.0)
    h *= L / h.sum()
    return h.reshape(P, L).T.astype(np.float32).copy(), L, M


def clean(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    bad = (x.view(np.uint32) & np.uint32(0x7FFFFFFF)) >= np.uint32(0x7F800000)
    return np.minimum(np.maximum(np.where(bad, F32(0.0), x), F32(-CLAMP)), F32(CLAMP))


def ceil_div(a, b):
    return -((-a) // b)


class Bank:
    """max_rows streams with one clock; push(x[nrows][n]) -> y[nrows][n_out], vectorised over the outputs, a loop over k"""

    def __init__(self, max_rows, L, M, taps):
        self.L, self.M = int(L), int(M)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(self.L, -1)
        self.P = self.taps.shape[1]
        self.hist = np.zeros((max_rows, self.P - 1), np.float32)
        self.nmod = 0
        self.frames_in = self.frames_out = 0

    def reset(self, row=-1):
        if row < 0:
            self.hist[:] = 0
            self.nmod = 0
            self.frames_in = self.frames_out = 0
        else:
            self.hist[row] = 0

    def out_frames(self, n):
        return ceil_div((self.nmod + n) * self.L, self.M) - ceil_div(self.nmod * self.L, self.M)

    def push(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        nrows, n = x.shape
        L, M, P, H, r = self.L, self.M, self.P, self.P - 1, self.nmod
        n_out = self.out_frames(n)
        j0 = ceil_div(r * L, M)
        u = (j0 + np.arange(n_out, dtype=np.int64)) * M
        rel, ph = u // L - r, u % L                            # n0 counted from the push's first frame; the phase
        assert n_out == 0 or (rel.min() >= 0 and rel.max() < n)
        ext = np.concatenate([self.hist[:nrows], clean(x)], axis=1)         # ext[:, H + i] is frame i of the push
        y = np.zeros((nrows, n_out), np.float32)
        for k in range(P):
            y = y + self.taps[ph, k][None, :] * ext[:, H + rel - k]
        if n:
            self.hist[:nrows] = ext[:, ext.shape[1] - H:]
            self.hist[nrows:] = 0                              # the rows a push leaves out saw nothing
        self.nmod = (r + n) % M
        self.frames_in += n
        self.frames_out += n_out
        return y


class LoopBank:
    """ONE row, the rule's lines one output and one tap at a time, on the whole stream since the last reset of all"""

    def __init__(self, L, M, taps):
        self.L, self.M = int(L), int(M)
        self.taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(self.L, -1)
        self.x = []                                            # cleaned frames since the clock's 0
        self.m = 0                                             # outputs so far

    def reset_row(self):
        self.x = [F32(0.0)] * len(self.x)

    def push(self, x):
        for v in np.asarray(x, dtype=np.float32).reshape(-1):
            bits = int(np.array([v], np.float32).view(np.uint32)[0])
            if (bits & 0x7FFFFFFF) >= 0x7F800000:
                v = F32(0.0)
            self.x.append(F32(min(max(v, F32(-CLAMP)), F32(CLAMP))))
        out = []
        while (self.m * self.M) // self.L < len(self.x):
            t = self.m * self.M
            n0, ph = t // self.L, t % self.L
            acc = F32(0.0)
            for k in range(self.taps.shape[1]):
                xv = self.x[n0 - k] if n0 - k >= 0 else F32(0.0)
                acc = F32(acc + F32(self.taps[ph, k] * xv))
            out.append(acc)
            self.m += 1
        return np.array(out, np.float32)
