"""-m gpu: wr_tuner_chan_levels / wr_iq_levels -- the signal level of every receiver of a tuner at the demodulator's input
(mean and peak of i*i + q*q over the last submit's channel IQ, and how many audio frames the squelch muted) from one
launch sequence.

The yardstick for every value is the channel IQ the same tuner hands out, t.fetch(ch, WR_STAGE_CHAN_IQ, ...): the bits
the kernels read.  mean and peak are compared BIT FOR BIT with the numpy float32 restatement of the header's rule of
summation (tests/levels_np.py, held to float64 in test_chan_levels_capi.py), muted with oracle.af_gain_squelch on a row of
ones.  Input: noise plus a carrier per receiver keyed on and off at 150 Hz, as test_gpu_f4.test_af_gain_and_squelch."""
import ctypes as C

import numpy as np
import pytest

import levels_np
from levels_np import bits
from rowcases import channel_ifs as _ifs, keyed_block as _block   # (at FS, the builder's default rate, unless told)
from webradio_amd import capi, synth
from webradio_amd.device import Tuner

pytestmark = pytest.mark.gpu

FS, CHAN_RATE, AUDIO_RATE, D1, D2 = 2_000_000, 5_000, 1_000, 400, 5
K1S = [1, 10, 15, 16, 17, 255, 256, 257, 600]


def _as_u8(iq):
    return np.clip(np.rint(iq * 128.0 + 128.0), 0, 255).astype(np.uint8)


def _tuner(dev, nrx, max_block, nco=capi.WR_NCO_EXACT, max_channels=None, mode=capi.WR_AM):
    t = Tuner(dev, FS, max_channels or nrx, max_block, nco)
    chans = [t.add_receiver(f, 128_000, CHAN_RATE, mode, 160, AUDIO_RATE) for f in _ifs(nrx)]
    return t, chans


def _muted_want(oracle, iq, d2, k2, sq):
    if sq is None or not k2:
        return 0, np.ones(k2, np.float32)
    gate = oracle.af_gain_squelch(np.ones(k2, np.float32), iq, d2, 0.0, sq)
    return int(np.count_nonzero(gate == 0.0)), gate


def _check(oracle, t, chans, levels, k1, d2, sq=None, what=""):
    """every channel's entry against its fetched channel IQ: the rule's bits, the peak, the gate's count"""
    mean, peak, muted, frames, audio_frames = levels
    assert frames == k1 and audio_frames == k1 // d2, what
    for n, ch in enumerate(chans):
        s = t.slot(ch)
        iq = t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1)
        assert iq.size == 2 * k1
        wm, wp = levels_np.levels(iq)
        assert float(wm) > 0.0, what
        print("%s slot %d mean %.9g (bits %08x, rule %08x) peak %.9g" % (what, s, mean[s], bits(mean[s]), bits(wm), peak[s]))
        assert bits(mean[s]) == bits(wm), (what, s)
        assert bits(peak[s]) == bits(wp), (what, s)
        want, _ = _muted_want(oracle, iq, d2, k1 // d2, sq[n] if sq else None)
        assert int(muted[s]) == want, (what, s)


# ---- 1, 2: the rule bit for bit, and against double ---------------------------------------------------------------------------

_rule_cache = {}


@pytest.fixture(scope="module")
def rule_case(dev):
    """rule_case(k1, nco, kind) -> (levels, {slot: fetched channel IQ}); each case run once, shared by the tests below"""
    def make(k1, nco, kind):
        key = (k1, nco, kind)
        if key not in _rule_cache:
            n = k1 * D1
            t, chans = _tuner(dev, 4, n, nco)
            iq = _block(n, _ifs(4), seed=k1, scale=10.0 if kind == "u8" else 1.0)
            if kind == "u8":
                t.submit_u8_host(_as_u8(iq))
            else:
                t.submit_host(iq)
            lv = t.chan_levels()
            iqs = {t.slot(ch): t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1) for ch in chans}
            t.destroy()
            _rule_cache[key] = (lv, iqs)
        return _rule_cache[key]
    yield make
    _rule_cache.clear()


_rule_params = [pytest.param(k1, nco, kind, id="%d-%s-%s" % (k1, "exact" if nco == capi.WR_NCO_EXACT else "rotate", kind))
                for k1 in K1S for nco in (capi.WR_NCO_EXACT, capi.WR_NCO_ROTATE) for kind in ("f32", "u8")]


@pytest.mark.parametrize("k1, nco, kind", _rule_params)
def test_the_rule_bit_for_bit(rule_case, k1, nco, kind):
    (mean, peak, muted, frames, audio_frames), iqs = rule_case(k1, nco, kind)
    assert frames == k1 and audio_frames == k1 // D2
    assert mean.size == peak.size == muted.size == 64
    for s, iq in iqs.items():
        assert iq.size == 2 * k1
        wm, wp = levels_np.levels(iq)
        print("K1 %d slot %d mean %.9g bits %08x rule %08x peak %.9g" % (k1, s, mean[s], bits(mean[s]), bits(wm), peak[s]))
        assert bits(mean[s]) == bits(wm)
        assert bits(peak[s]) == bits(wp) == bits(levels_np.power(iq).max())
        assert muted[s] == 0                                   # no squelch in use


@pytest.mark.parametrize("k1, nco, kind", _rule_params)
def test_against_double(rule_case, k1, nco, kind):
    (mean, _, _, _, _), iqs = rule_case(k1, nco, kind)
    for s, iq in iqs.items():
        want = levels_np.mean_f64(iq)
        assert want > 0.0                                      # a non-zero mean in every used slot
        rel = abs(float(mean[s]) - want) / want
        print("K1 %d slot %d relative error %.3g, bound %.3g" % (k1, s, rel, levels_np.mean_bound(k1)))
        assert rel <= levels_np.mean_bound(k1)


# ---- 3: two lane groups ---------------------------------------------------------------------------------------------------------

def test_two_lane_groups(dev, oracle):
    k1 = 257
    n = k1 * D1
    iq = _block(n, _ifs(70)[::9], seed=3)
    t, chans = _tuner(dev, 70, n)
    t.submit_host(iq)
    first = t.chan_levels()
    assert first[0].size == first[1].size == first[2].size == 128
    assert sorted(t.slot(ch) for ch in chans) == list(range(70))
    _check(oracle, t, chans, first, k1, D2, what="70 receivers")
    again = t.chan_levels()
    for a, b in zip(first[:3], again[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    t.destroy()


def test_the_same_bits_whatever_max_channels(dev):
    k1 = 257
    n = k1 * D1
    iq = _block(n, _ifs(8), seed=4)
    got = []
    for max_channels in (8, 70):
        t, chans = _tuner(dev, 8, n, max_channels=max_channels)
        t.submit_host(iq)
        mean, peak, muted, _, _ = t.chan_levels()
        used = [t.slot(ch) for ch in chans]
        assert float(mean[used].min()) > 0.0
        got.append((mean[used], peak[used], muted[used]))
        t.destroy()
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 4: the gate ------------------------------------------------------------------------------------------------------------------

def _clear_of_threshold(iq, d2, k2, sq):
    """no audio frame's mean power (float64) within a relative 1e-5 of the threshold: a last bit cannot decide a frame"""
    z = np.asarray(iq, np.float64).reshape(-1, 2)[: k2 * d2]
    p = (z[:, 0] ** 2 + z[:, 1] ** 2).reshape(k2, d2).mean(axis=1)
    thr = 10.0 ** (sq / 10.0)
    return float(np.abs(p - thr).min()) > 1e-5 * thr


def test_the_gate(dev, oracle):
    k1 = 600
    k2 = k1 // D2
    n = k1 * D1
    sqs = [-46.0, -44.0, -48.0, None]
    t, chans = _tuner(dev, 4, n)
    for ch, sq in zip(chans, sqs):
        t.set_squelch(ch, sq if sq is not None else 0.0, sq is not None)
    t.submit_host(_block(n, _ifs(4), seed=5))
    lv = t.chan_levels()
    _check(oracle, t, chans, lv, k1, D2, sq=sqs, what="gate")
    muted = lv[2]
    for ch, sq in zip(chans, sqs):
        s = t.slot(ch)
        if sq is None:
            assert muted[s] == 0
            continue
        iq = t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1)
        assert _clear_of_threshold(iq, D2, k2, sq)
        assert 0 < muted[s] < k2                                # the gate really opens and closes
        _, gate = _muted_want(oracle, iq, D2, k2, sq)
        audio = t.fetch(ch, capi.WR_STAGE_AUDIO, k2)
        assert audio.size == k2 and np.all(audio[gate == 0.0] == 0.0)
    # a threshold staged after the block shows once a block has been submitted with it
    before = muted.copy()
    t.set_squelch(chans[0], -90.0, True)
    t.set_squelch(chans[3], -44.0, True)
    assert np.array_equal(t.chan_levels()[2], before)
    t.submit_host(_block(n, _ifs(4), seed=6, pos=n))
    sqs2 = [-90.0, -44.0, -48.0, -44.0]
    lv2 = t.chan_levels()
    for ch, sq in zip(chans, sqs2):
        assert _clear_of_threshold(t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1), D2, k2, sq)
    _check(oracle, t, chans, lv2, k1, D2, sq=sqs2, what="gate, next block")
    assert lv2[2][t.slot(chans[0])] == 0 and 0 < lv2[2][t.slot(chans[3])] < k2
    t.destroy()


# ---- 5: other paths -------------------------------------------------------------------------------------------------------------

def test_with_a_second_channel_stage(dev, oracle):
    """2 M -> 50 k -> 5 k -> 1 k: the levels are those of the second stage's output, what fetch(CHAN_IQ) returns there"""
    k1 = 257
    n = k1 * D1
    sqs = [-46.0, None, -46.0]
    t = Tuner(dev, FS, 3, n, capi.WR_NCO_EXACT)
    chans = [t.add_receiver(f, 250_000, 50_000, capi.WR_AM, 160, AUDIO_RATE, stage2=(64, 2_000, CHAN_RATE)) for f in _ifs(3)]
    for ch, sq in zip(chans, sqs):
        t.set_squelch(ch, sq if sq is not None else 0.0, sq is not None)
    t.submit_host(_block(n, _ifs(3), seed=7))
    _check(oracle, t, chans, t.chan_levels(), k1, D2, sq=sqs, what="second stage")
    t.destroy()


def test_with_the_demodulator_output_kept(dev, oracle):
    k1 = 257
    n = k1 * D1
    sqs = [-46.0, None, -44.0]
    t, chans = _tuner(dev, 3, n)
    t.keep_stages(capi.WR_STAGE_DEMOD)
    for ch, sq in zip(chans, sqs):
        t.set_squelch(ch, sq if sq is not None else 0.0, sq is not None)
    t.submit_host(_block(n, _ifs(3), seed=8))
    _check(oracle, t, chans, t.chan_levels(), k1, D2, sq=sqs, what="demod kept")
    t.destroy()


def test_an_audio_decimation_outside_the_fused_set(dev, oracle):
    fs, d1, d2, k1 = 2_100_000, 300, 7, 257                       # 2.1 M -> 7 k -> 1 k
    n = k1 * d1
    sqs = [-46.0, None, -44.0]
    t = Tuner(dev, fs, 3, n, capi.WR_NCO_EXACT)
    chans = [t.add_receiver(f, 128_000, 7_000, capi.WR_AM, 160, 1_000) for f in _ifs(3)]
    for ch, sq in zip(chans, sqs):
        t.set_squelch(ch, sq if sq is not None else 0.0, sq is not None)
    t.submit_host(_block(n, _ifs(3), seed=9, fs=fs))
    _check(oracle, t, chans, t.chan_levels(), k1, d2, sq=sqs, what="d2 = 7")
    t.destroy()


# the streaming launch takes the shape test_gpu_chan_spectra streams: FM off 2.4 Msps, 240 kHz channels, 48 kHz audio
SFS, SCHAN, SAUDIO, SD1, SNRX = 2_400_000, 240_000, 48_000, 10, 70


def _s_ifs(nrx=SNRX):
    return [(c - nrx // 2) * 30_000 + 99 for c in range(nrx)]


def _s_stream(nframes, seed):
    return synth.fm_stream(nframes, SFS, _s_ifs()[3::16], amp=0.1, fm_base=700.0, fm_step=900.0, beta=2.0,
                           noise_dbfs=-50, seed=seed)


def _s_tuner(dev, max_block):
    t = Tuner(dev, SFS, SNRX, max_block, capi.WR_NCO_ROTATE)
    chans = [t.add_receiver(f, 100_000, SCHAN, capi.WR_FM, 8_000, SAUDIO) for f in _s_ifs()]
    return t, chans


def test_after_a_streaming_launch(dev, oracle):
    """three device-resident blocks into a streaming launch, then the call: it closes the launch and reads the launch's
    own ring; the values are the bits of the same blocks on a tuner that launches per block"""
    k1 = 640
    n = k1 * SD1
    x = dev.upload(_s_stream(3 * n, seed=10))
    got = {}
    for stream in (False, True):
        t, chans = _s_tuner(dev, n)
        t.streaming(stream)
        for b in range(3):
            t.submit_device(x + 8 * n * b, n)
        assert t.stream_info()[0] is stream
        lv = t.chan_levels()
        assert t.stream_info()[0] is False
        if stream:
            assert t.stream_info()[2] == 3
        _check(oracle, t, chans, lv, k1, 5, what="streaming" if stream else "per block")
        used = [t.slot(ch) for ch in chans]
        got[stream] = (lv[0][used], lv[1][used], lv[2][used])
        t.destroy()
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    dev.free(x)


# ---- 6: nothing is disturbed ----------------------------------------------------------------------------------------------------

def test_asking_disturbs_nothing(dev):
    k1 = 257
    n = k1 * D1
    sqs = [-46.0, None, -44.0, None]
    twins = []
    for _ in range(2):
        t, chans = _tuner(dev, 4, n, nco=capi.WR_NCO_ROTATE)
        for ch, sq in zip(chans, sqs):
            t.set_squelch(ch, sq if sq is not None else 0.0, sq is not None)
        twins.append((t, chans))
    for b in range(4):
        iq = _block(n, _ifs(4), seed=20 + b, pos=b * n)
        out = []
        for asked, (t, chans) in enumerate(twins):
            t.submit_host(iq)
            if asked:
                assert float(t.chan_levels()[0][: len(chans)].min()) > 0.0
            out.append((t.fetch_audio_all(), [t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1) for ch in chans],
                        [t.state(ch) for ch in chans]))
        (a0, c0, s0), (a1, c1, s1) = out
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), b
        for x0, x1 in zip(c0, c1):
            assert np.array_equal(x0.view(np.uint32), x1.view(np.uint32)), b
        for (p0, v0), (p1, v1) in zip(s0, s1):
            assert p0 == p1 and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)), b
    for t, _ in twins:
        t.destroy()


def test_asking_disturbs_nothing_while_streaming(dev):
    k1 = 640
    n = k1 * SD1
    x = dev.upload(_s_stream(4 * n, seed=11))
    rings, launches, last = [], [], []
    for asked in (False, True):
        t, chans = _s_tuner(dev, n)
        t.audio_ring(4)
        t.streaming(True)
        for b in range(4):
            t.submit_device(x + 8 * n * b, n)
            if asked:
                assert t.chan_levels()[3] == k1
        t.flush()
        entries = []
        for b in range(4):
            audio, seq = t.ring_acquire()
            assert seq == b
            entries.append(audio.copy())
            t.ring_release()
        rings.append(entries)
        launches.append(t.stream_info()[1])
        last.append([t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1) for ch in chans] + [t.state(ch)[1] for ch in chans])
        t.destroy()
    for b in range(4):
        assert np.array_equal(rings[0][b].view(np.uint32), rings[1][b].view(np.uint32)), b
    for a, b in zip(*last):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert launches[1] > launches[0] >= 1
    dev.free(x)


# ---- 7: errors ------------------------------------------------------------------------------------------------------------------

def test_errors(dev):
    lib = dev.lib
    k1 = 16
    n = k1 * D1
    out = np.zeros(64, np.float32)
    t, chans = _tuner(dev, 2, n, max_channels=3)
    call = lib.wr_tuner_chan_levels
    assert call(t.h, capi.ptr(out), None, None, None, None, None) == capi.WR_ERR_STATE
    assert b"nothing submitted" in lib.wr_last_error()
    t.submit_host(_block(n, _ifs(2), seed=12))
    assert call(t.h, None, None, None, None, None, None) == capi.WR_ERR_ARG
    frames, slots = C.c_size_t(), C.c_uint()
    assert call(t.h, None, capi.ptr(out), None, C.byref(frames), None, C.byref(slots)) == capi.WR_OK
    assert frames.value == k1 and slots.value == 64 and float(out[:2].min()) > 0.0
    t.add_receiver(5_000, 128_000, 10_000, capi.WR_AM, 160, 2_000)          # a second rate group
    assert call(t.h, capi.ptr(out), None, None, None, None, None) == capi.WR_ERR_STATE
    assert b"several rate groups" in lib.wr_last_error()
    t.destroy()
    x = dev.upload(np.ones(8, np.float32))
    m = C.c_float()
    assert lib.wr_iq_levels(dev.h, C.c_void_p(x), 0, C.byref(m), None) == capi.WR_ERR_ARG
    assert lib.wr_iq_levels(dev.h, None, 4, C.byref(m), None) == capi.WR_ERR_ARG
    dev.free(x)


# ---- 8: a plain block -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 17, 257, 4097])
def test_iq_levels(dev, k):
    iq = (0.1 * np.random.default_rng(k).standard_normal(2 * k)).astype(np.float32)
    x = dev.upload(iq)
    calls = dev.lib.wr_block_kernel_calls()
    mean, peak = dev.iq_levels(x, k)
    assert dev.lib.wr_block_kernel_calls() == calls + 1
    wm, wp = levels_np.levels(iq)
    assert bits(mean) == bits(wm) and bits(peak) == bits(wp)
    dev.free(x)
