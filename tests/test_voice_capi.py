"""The voice bank without a GPU: the nine functions are declared and bound with the same argument counts, the header carries
the rule, NULL handles are refused by name, wr_voice_design gives numpy's numbers and filters that meet the stated
conditions, and the restatement the GPU tests compare bits with (tests/voice_np.py) is held here first to the rule written
as plain loops (bit for bit, for any cut into pushes), to an ideal sine delayed by the group delay and to a unit-impulse
filter."""
import ctypes as C
import re

import numpy as np
import pytest

import capicases
import voice_np
from resamp_np import clean
from webradio_amd import capi

NAMES = [("wr_voice_design", 6), ("wr_voice_create", 6), ("wr_voice_destroy", 1), ("wr_voice_reset", 2), ("wr_voice_set_rows", 4),
         ("wr_voice_get_rows", 4), ("wr_voice_push_rows", 7), ("wr_tuner_voice_push", 5), ("wr_voice_info", 4)]
# (audio_rate, T, highpass_hz, lowpass_hz, deemph_us)
DESIGNS = [(50_000, 1024, 300, 3000, 750), (50_000, 2048, 300, 3000, 750), (32_000, 1024, 300, 3000, 750),
           (16_000, 512, 300, 3000, 0), (8_000, 256, 300, 3400, 0), (50_000, 1024, 300, 0, 0)]
SPECIAL = [np.inf, -np.inf, np.nan, 1e30, -1e30, -0.0, 1e-40, 65536.0]
MUTE = voice_np.MUTE


# ---- 1: declared and bound ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, nargs", NAMES)
def test_declared_and_bound_with_the_same_arguments(name, nargs):
    capicases.declared_and_bound(name, nargs)


def test_header_says_the_rule():
    text = capicases.header()
    assert re.search(r"#define\s+WR_ABI_VERSION\s+6\b", text)
    assert re.search(r"Added to 6 later: wr_voice_design, wr_voice_create, wr_voice_destroy, wr_voice_reset,\s+"
                     r"wr_voice_set_rows, wr_voice_get_rows, wr_voice_push_rows,\s+wr_tuner_voice_push, wr_voice_info\.", text)
    rule = text[text.index("VOICE BANK:"):]
    for word in ("x'   = 0.0f if (bits(x) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else min(max(x, -65536.0f), 65536.0f)",
                 "acc  = +0.0f", "for k = 0 ... T-1 in this order:  acc = acc + c[f][k] * x'[n - k]", "y[n] = mute ? +0.0f : acc",
                 "from 1 to 65535", "from 1 to 16", "a multiple of 4 from 8", "to 2048", "|c| <= 16", "bits 0-7", "bit 8 is the mute flag",
                 "at most 2^28 frames", "may not overlap", "recursive filters", "per-row filter lengths",
                 "inside the streaming launch", "host-side C++", "an int16 output", "time sharding", "both orders work",
                 "G = 32768", "beta = 6", "only -40 dB"):
        assert word in rule, word


def test_the_package_exports_the_names():
    import webradio_amd
    from webradio_amd import device
    assert webradio_amd.VoiceBank is device.VoiceBank and webradio_amd.voice_design is device.voice_design
    assert "VoiceBank" in webradio_amd.__all__ and "voice_design" in webradio_amd.__all__
    assert hasattr(device.Tuner, "voice_push")
    for method in ("set_rows", "get_rows", "push_rows", "reset", "info", "destroy"):
        assert hasattr(device.VoiceBank, method), method


def test_null_handles_are_refused():
    lib = capi.load()
    a = np.zeros(16, np.float32)
    w = np.zeros(4, np.uint32)
    h = C.c_void_p()
    for call, name in ((lambda: lib.wr_voice_create(C.byref(h), None, 1, 8, 1, capi.ptr(a)), b"wr_voice_create"),
                       (lambda: lib.wr_voice_create(None, None, 1, 8, 1, capi.ptr(a)), b"wr_voice_create"),
                       (lambda: lib.wr_voice_create(C.byref(h), None, 1, 8, 1, None), b"wr_voice_create"),
                       (lambda: lib.wr_voice_reset(None, -1), b"wr_voice_reset"),
                       (lambda: lib.wr_voice_set_rows(None, 0, 1, capi.ptr(w)), b"wr_voice_set_rows"),
                       (lambda: lib.wr_voice_get_rows(None, 0, 1, capi.ptr(w)), b"wr_voice_get_rows"),
                       (lambda: lib.wr_voice_push_rows(None, capi.ptr(a), 4, 1, 4, capi.ptr(a), 4), b"wr_voice_push_rows"),
                       (lambda: lib.wr_tuner_voice_push(None, None, None, 0, None), b"wr_tuner_voice_push"),
                       (lambda: lib.wr_voice_info(None, None, None, None), b"wr_voice_info"),
                       (lambda: lib.wr_voice_design(16_000, 512, 300, 3000, 0, None), b"wr_voice_design")):
        assert call() == capi.WR_ERR_ARG, name
        assert name in lib.wr_last_error(), (name, lib.wr_last_error())
    assert lib.wr_voice_destroy(None) == capi.WR_OK


# ---- 2 - 4: the design helper ---------------------------------------------------------------------------------------------------

def _design(audio_rate, T, hp, lp, de, room=2304):
    taps = np.full(room, np.float32(np.nan), np.float32)
    rc = capi.load().wr_voice_design(audio_rate, T, hp, lp, de, capi.ptr(taps))
    return rc, taps


@pytest.mark.parametrize("audio_rate, T, hp, lp, de", DESIGNS)
def test_design_equals_numpy(audio_rate, T, hp, lp, de):
    want = voice_np.design(audio_rate, T, hp, lp, de)
    rc, taps = _design(audio_rate, T, hp, lp, de)
    assert rc == capi.WR_OK
    got = taps[:T]
    assert np.isnan(taps[T:]).all()                                       # nothing written behind [T]
    # two evaluations of the same double formula, each rounded to float32 once
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print("%d Hz, T %d, %d .. %d Hz, %d us: max |c| %.4f, max difference %.3g" % (audio_rate, T, hp, lp, de, np.abs(want).max(), err))
    assert err <= 2.0 ** -23 * np.abs(want).max()
    assert got[T - 1] == 0.0 and not np.signbit(got[T - 1])               # tap T - 1 is +0.0f
    assert np.array_equal(got[: T - 1].view(np.uint32), got[: T - 1][::-1].view(np.uint32))     # h[i] and h[T - 2 - i]: the same bits
    assert np.abs(got).max() <= 16.0


def _quality(taps, audio_rate, T, hp, lp, de):
    """(low stopband, high stopband or None, passband deviation) in dB, from float taps in float64"""
    nfft = 1 << 18
    mag = np.abs(np.fft.rfft(taps.astype(np.float64), nfft))
    f = np.arange(mag.size) * (audio_rate / nfft)
    W = voice_np.half_width(audio_rate, T)
    low = 20 * np.log10(mag[f <= hp - W].max())
    high = 20 * np.log10(mag[f >= lp + W].max()) if lp else None
    inside = (f >= hp + W) & (f <= (lp - W if lp else audio_rate / 2.0))
    want = voice_np.desired(audio_rate, f[inside], hp, lp, de)
    dev = 20 * np.log10(np.abs(mag[inside] / want - 1.0).max())
    return low, high, dev


@pytest.mark.parametrize("audio_rate, T, hp, lp, de", DESIGNS)
def test_design_quality(audio_rate, T, hp, lp, de):
    """From the C helper's float taps, in float64, with a zero-padded FFT of 2^18 points: |H| <= -55 dB for
    f <= highpass_hz - W and for f >= lowpass_hz + W; |H / D - 1| <= -45 dB for highpass_hz + W <= f <= lowpass_hz - W (up
    to rate / 2 without a low-pass).  Found with voice_np.design's taps (low stopband, high stopband, passband deviation, dB):
        50000 / 1024, 750 us   -58.9  -76.8  -47.9
        50000 / 2048, 750 us   -58.8  -76.2  -56.8
        32000 / 1024, 750 us   -61.3  -74.7  -54.2
        16000 / 512            -69.4  -69.4  -69.0
        8000 / 256             -69.5  -68.6  -69.1
        50000 / 1024, high-pass -67.6 (none) -68.7"""
    rc, taps = _design(audio_rate, T, hp, lp, de)
    assert rc == capi.WR_OK
    low, high, dev = _quality(taps[:T], audio_rate, T, hp, lp, de)
    ref = _quality(voice_np.design(audio_rate, T, hp, lp, de), audio_rate, T, hp, lp, de)
    print("%d Hz, T %d, %d .. %d Hz, %d us: low stopband %.1f dB, high stopband %s dB, passband deviation %.1f dB "
          "(voice_np: %.1f, %s, %.1f)" % (audio_rate, T, hp, lp, de, low, "%.1f" % high if lp else "(none)", dev, ref[0],
                                         "%.1f" % ref[1] if lp else "(none)", ref[2]))
    assert low <= -55.0
    assert high is None or high <= -55.0
    assert dev <= -45.0


@pytest.mark.parametrize("audio_rate, T, hp, lp, de", [(0, 512, 300, 3000, 0),           # a rate of 0
                                                       (16_000, 0, 300, 3000, 0), (16_000, 4, 300, 3000, 0),
                                                       (16_000, 510, 300, 3000, 0), (16_000, 2052, 300, 3000, 0),
                                                       (16_000, 512, 300, 8000, 0),      # lowpass_hz = rate / 2
                                                       (16_000, 512, 300, 9000, 0),
                                                       (16_000, 512, 300, 500, 0),       # 300 + W >= 500 - W: W is 120 Hz
                                                       (16_000, 512, 3000, 300, 0),
                                                       (50_000, 1024, 300, 3000, 10_001)])
def test_design_refuses(audio_rate, T, hp, lp, de):
    rc, taps = _design(audio_rate, T, hp, lp, de)
    assert rc == capi.WR_ERR_ARG
    assert b"wr_voice_design" in capi.load().wr_last_error()
    assert np.isnan(taps).all()                                           # ... and nothing was written


def test_design_edges_just_far_enough():
    """the edge rule is highpass_hz + W >= lowpass_hz - W: 300 .. 542 Hz at 16 kHz / 512 (W = 120.5) passes, 300 .. 540 does not"""
    W = voice_np.half_width(16_000, 512)
    assert 300 + W < 542 - W and 300 + W >= 540 - W
    assert _design(16_000, 512, 300, 542, 0)[0] == capi.WR_OK
    assert _design(16_000, 512, 300, 540, 0)[0] == capi.WR_ERR_ARG
    assert _design(50_000, 8, 0, 0, 10_000)[0] == capi.WR_OK              # the limits themselves pass
    assert _design(50_000, 2048, 0, 24_999, 0)[0] == capi.WR_OK


# ---- 5: the restatement against the rule as plain loops -------------------------------------------------------------------------

def _rough_taps(F, T, seed):
    """random taps in +-16 with -0.0, subnormals and 16.0 among them"""
    taps = np.random.default_rng(seed).uniform(-16.0, 16.0, (F, T)).astype(np.float32)
    taps[0, 0], taps[1, 3], taps[2, T - 1], taps[2, 2] = -0.0, 1e-40, -1e-42, 16.0
    return taps


@pytest.mark.parametrize("T", [8, 64])
def test_the_restatement_is_the_loop(T):
    """three rows on different filters, one of them muted; pushes of 1, T - 2, T - 1, 0 and more frames; a reset of one row
    in mid-stream, a push that leaves a row out, a filter index changed between pushes, mute switched on and off.  Each
    row against its own loop; and the frames of a row that is not muted equal those of a twin bank that never was."""
    F, n = 3, 3 * T + 200
    taps = _rough_taps(F, T, seed=T)
    v = np.stack([capicases.audio(n, 10 * T + r, SPECIAL, 7) for r in range(3)])
    bank, twin = voice_np.Bank(3, taps), voice_np.Bank(3, taps)
    loops = [voice_np.LoopBank(taps) for _ in range(3)]
    pos = 0

    def words(w):
        bank.set_rows(0, w)
        twin.set_rows(0, [x & 0xFF for x in w])
        for r in range(3):
            loops[r].word = w[r]

    def push(length, nrows=3):
        nonlocal pos
        y = bank.push(v[:nrows, pos: pos + length])
        z = twin.push(v[:nrows, pos: pos + length])
        assert y.shape == (nrows, length)
        for r in range(nrows):
            assert capicases.same_bits(y[r], loops[r].push(v[r, pos: pos + length])), (T, r, pos, length)
            if bank.ctl[r] & MUTE:
                assert not y[r].view(np.uint32).any()                     # +0.0f, every frame
            else:
                assert capicases.same_bits(y[r], z[r]), (T, r, pos, length)
        for r in range(nrows, 3):                                         # a row left out saw nothing
            loops[r].reset_row()
        pos += length

    words([0, 1 | MUTE, 2])
    for length in (1, T - 2, T - 1, 0, 30):
        push(length)
    bank.reset(0)
    twin.reset(0)
    loops[0].reset_row()
    push(20)
    push(10, nrows=2)
    assert not bank.hist[2].any()
    words([2, 1 | MUTE, 2])                                               # row 0: new taps on the old inputs
    push(25)
    words([2, 1, 2])                                                      # row 1 speaks: the frames it would have given
    push(25)
    words([2, 1, 0 | MUTE])
    push(T + 3)
    words([2, 1, 0])
    push(n - pos)
    assert bank.frames == n and np.abs(bank.push(v[:, :1])).max() <= 2.0 ** 31


# ---- 6: a tone comes out delayed -----------------------------------------------------------------------------------------------

def test_a_tone_comes_out_delayed():
    """A 1 kHz tone at 16 kHz through the C helper's design(16000, 512, 300, 3000, 0) comes out as the ideal sine delayed by
    exactly T / 2 - 1 frames, within 1e-3 (the -45 dB passband condition, 5.6e-3, with margin: the design keeps -69 dB),
    behind the first T outputs; a 100 Hz tone comes out below 1e-2 of its amplitude (loose: the -55 dB stopband condition
    from highpass_hz - W = 180 Hz down gives 1.8e-3)."""
    rate, T = 16_000, 512
    rc, taps = _design(rate, T, 300, 3000, 0)
    assert rc == capi.WR_OK
    n = np.arange(3 * T, dtype=np.float64)
    for hz, what in ((1000.0, "pass"), (100.0, "stop")):
        x = np.sin(2 * np.pi * hz * n / rate).astype(np.float32)
        bank = voice_np.Bank(1, taps[:T])
        y = np.concatenate([bank.push(x[None, :700])[0], bank.push(x[None, 700:])[0]])
        ideal = np.sin(2 * np.pi * hz * (n - (T // 2 - 1)) / rate)
        if what == "pass":
            err = np.abs(y[T:] - ideal[T:]).max()
            print("1 kHz: largest error %.3g over %d outputs" % (err, y.size - T))
            assert err <= 1e-3
        else:
            left = np.abs(y[T:]).max()
            print("100 Hz: %.3g of its amplitude is left" % left)
            assert left <= 1e-2


# ---- 7: a unit-impulse filter ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [8, 64, 512])
def test_a_unit_impulse_filter_delays(T):
    """c[T / 2 - 1] = 1 and 0 elsewhere returns clean(x) delayed by T / 2 - 1 frames, bit for bit -- but for a -0.0 input,
    which the rule turns into +0.0: the accumulator starts at +0.0f, and (+0) + (-0) = +0"""
    d = T // 2 - 1
    taps = np.zeros(T, np.float32)
    taps[d] = 1.0
    x = capicases.audio(2 * T + 50, T, SPECIAL, 7)
    assert np.signbit(x[x == 0]).any()
    bank = voice_np.Bank(1, taps)
    y = np.concatenate([bank.push(x[None, :T - 3])[0], bank.push(x[None, T - 3:])[0]])
    want = np.concatenate([np.zeros(d, np.float32), clean(x)[: x.size - d]])
    want = np.where(want == 0, np.float32(0.0), want)                     # -0.0 -> +0.0
    assert capicases.same_bits(y, want)
