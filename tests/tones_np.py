"""The tone bank's rule (include/webradio_amd.h: TONE BANK) restated in vectorised numpy with int64 sums -- what the GPU tests
compare bits with.  test_tones_capi.py holds it to the rule written as plain loops and to a float64 DFT.

    w  = min(max(v', -64), 64) * 2^24, v' = 0 for an inf or a NaN
    p  = (uint32)(j * step),  i = p >> 20,  s = T12[i],  c = T12[(i + 1024) & 4095],  T12[i] = wr_sin_table()[16 i]
    I += (int64)rint(w * c),  Q += (int64)rint(w * s),  E += ((int64)rint(w))^2 >> 14

Bank is the streaming behaviour: pushes of any length, the latch at a window's last frame, the window count, the fill."""
import ctypes as C

import numpy as np

from webradio_amd import capi

_T12 = None


def table12():
    """T12[4096]: every 16th entry of the library's sine table (wr_sin_table needs no device)"""
    global _T12
    if _T12 is None:
        t = np.zeros(65536, np.float32)
        assert capi.load().wr_sin_table(capi.ptr(t)) == capi.WR_OK
        _T12 = t[::16].copy()
    return _T12


def step_of(hz, audio_rate):
    """llround(hz / audio_rate * 2^32): half away from zero, as C's llround (np.rint would round half to even)"""
    x = np.float64(hz) / np.float64(audio_rate) * np.float64(4294967296.0)
    lo = np.floor(x)
    return int(lo) + (1 if x - lo >= 0.5 else 0)


def clean(v):
    """v': an inf or a NaN counts as 0, the rest is clamped to +-64 (float32)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    bad = (v.view(np.uint32) & np.uint32(0x7FFFFFFF)) >= np.uint32(0x7F800000)
    return np.minimum(np.maximum(np.where(bad, np.float32(0.0), v), np.float32(-64.0)), np.float32(64.0))


def quantise(v):
    """w (float32, exact)"""
    return clean(v) * np.float32(16777216.0)


def sums(v, steps, j0=0):
    """(I[ntones], Q[ntones], E) of frames j0, j0 + 1, ... of ONE window with audio values v"""
    t12 = table12()
    w = quantise(v)
    steps = np.asarray(steps, dtype=np.uint64)
    j = np.arange(j0, j0 + w.size, dtype=np.uint64)
    p = (j[:, None] * steps[None, :]) & np.uint64(0xFFFFFFFF)
    i = (p >> np.uint64(20)).astype(np.int64)
    s, c = t12[i], t12[(i + 1024) & 4095]
    I = np.rint(w[:, None] * c).astype(np.int64).sum(axis=0)              # float32 products, rounded once
    Q = np.rint(w[:, None] * s).astype(np.int64).sum(axis=0)
    qv = np.rint(w).astype(np.int64)
    return I, Q, int(((qv * qv) >> 14).sum())


class Bank:
    """max_rows independent streams; push(x[nrows][n]) continues rows 0 .. nrows-1"""

    def __init__(self, max_rows, steps, window):
        self.steps = np.asarray(steps, dtype=np.uint32)
        self.window = int(window)
        n = self.steps.size
        self.acc = np.zeros((max_rows, n, 2), np.int64)
        self.acc_e = np.zeros(max_rows, np.int64)
        self.iq = np.zeros((max_rows, n, 2), np.int64)
        self.energy = np.zeros(max_rows, np.int64)
        self.windows = np.zeros(max_rows, np.uint64)
        self.fill = np.zeros(max_rows, np.uint32)

    def reset(self, row=-1):
        rows = slice(None) if row < 0 else row
        for a in (self.acc, self.acc_e, self.iq, self.energy, self.windows, self.fill):
            a[rows] = 0

    def push(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        for r in range(x.shape[0]):
            pos, n = 0, x.shape[1]
            while pos < n:
                f = int(self.fill[r])
                take = min(self.window - f, n - pos)
                I, Q, E = sums(x[r, pos: pos + take], self.steps, f)
                self.acc[r, :, 0] += I
                self.acc[r, :, 1] += Q
                self.acc_e[r] += E
                pos += take
                if f + take == self.window:
                    self.iq[r], self.energy[r] = self.acc[r], self.acc_e[r]
                    self.acc[r], self.acc_e[r] = 0, 0
                    self.windows[r] += np.uint64(1)
                    self.fill[r] = 0
                else:
                    self.fill[r] = f + take

    def read(self):
        return self.iq, self.energy, self.windows, self.fill


def ratios(iq, energy, window):
    """rho = 2 (I^2 + Q^2) / (W E 2^14) in float64; 0 where E is 0"""
    i, q = iq[..., 0].astype(np.float64), iq[..., 1].astype(np.float64)
    den = (float(window) * np.asarray(energy, dtype=np.float64) * 16384.0)[..., None]
    out = np.zeros(i.shape, np.float64)
    np.divide(2.0 * (i * i + q * q), den, out=out, where=den > 0)
    return out


# ---- the tuner test's signal: FM carriers that carry a CTCSS tone and a 400 Hz tone of twice the deviation ---------------------

FS, CHAN_RATE, AUDIO_RATE = 2_000_000, 5_000, 1_000
CHAN_PASSBAND, AUDIO_PASSBAND = 128_000, 1_000
TONED = (67.0, 100.0, 151.4, 254.1)                # receivers 0 .. 3; receiver 4 carries the 400 Hz tone alone
VOICE_HZ, CTCSS_DEV, VOICE_DEV = 400.0, 300.0, 600.0
IFS = (-400_321, -200_123, 77, 200_211, 400_433)
CARRIER = 0.15


def fm_block(nframes, pos=0, seed=11):
    """interleaved float32 IQ of frames [pos, pos + nframes) of the five carriers plus a little noise"""
    t = (np.arange(nframes, dtype=np.float64) + pos) / FS
    z = np.zeros(nframes, np.complex128)
    for r, f in enumerate(IFS):
        ph = 2 * np.pi * ((f * t) % 1.0) + VOICE_DEV / VOICE_HZ * np.sin(2 * np.pi * VOICE_HZ * t)
        if r < len(TONED):
            ph = ph + CTCSS_DEV / TONED[r] * np.sin(2 * np.pi * TONED[r] * t)
        z += CARRIER * np.exp(1j * ph)
    rng = np.random.default_rng(seed + pos)
    z += 0.001 * (rng.standard_normal(nframes) + 1j * rng.standard_normal(nframes))
    out = np.empty(2 * nframes, np.float32)
    out[0::2], out[1::2] = z.real, z.imag
    return out


def detection(rho, tones_hz):
    """the detection conditions on rho[5][ntones]: (own / largest other per toned receiver, the untoned receiver's largest
    rho over the smallest own-tone rho); the conditions are: every first >= 4, the second < 1/4"""
    tones_hz = list(tones_hz)
    margins, owns = [], []
    for r, hz in enumerate(TONED):
        own = tones_hz.index(hz)
        assert int(np.argmax(rho[r])) == own, (r, hz, int(np.argmax(rho[r])))
        margins.append(rho[r, own] / np.delete(rho[r], own).max())
        owns.append(rho[r, own])
    return margins, rho[len(TONED)].max() / min(owns)
