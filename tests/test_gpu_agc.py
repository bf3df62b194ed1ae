"""-m gpu: the audio AGC -- wr_agc_rows on plain rows and wr_chan_set_agc inside a tuner -- BIT FOR BIT against the numpy
restatement of the header's rule (tests/agc_np.py, held to the rule's plain loop in test_agc_capi.py).

Inputs of the bit comparisons are zeros and normal floats: bursts 80 dB apart, runs of exact zeros, negative values, no
denormals; one extra case holds an inf and a NaN.  In the tuner tests the yardstick for a receiver WITH AGC is the audio
v of a twin tuner with scale 1 and gains of 0 dB, put through agc_np.apply and carried from block to block; for a
receiver WITHOUT AGC it is the audio of a twin with no AGC anywhere, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import agc_np
from agc_np import OFF, bits
from rowcases import channel_ifs as _ifs, keyed_block as _block   # (at FS, the builder's default rate)
from webradio_amd import capi
from webradio_amd.device import Tuner, agc_design

pytestmark = pytest.mark.gpu

FS, CHAN_RATE, AUDIO_RATE, D1, D2 = 2_000_000, 5_000, 1_000, 400, 5
MODES = [capi.WR_AM, capi.WR_FM, capi.WR_USB, capi.WR_LSB]
TINY = np.finfo(np.float32).tiny
SCALE = 32768.0


def _rows(nrows, n, seed):
    """bursts decades (up to 80 dB) apart, runs of exact zeros, negative values; no denormals"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((nrows, n)) * 10.0 ** rng.integers(-4, 1, (nrows, n))).astype(np.float32)
    v[rng.random((nrows, n)) < 0.2] = 0.0
    if n > 40:
        v[:, n // 3: n // 3 + 17] = 0.0
    assert not np.any((v != 0) & (np.abs(v) < TINY))
    return v


def _params(nrows):
    """per row: a target, a floor, a step -- every third row (from row 2) without AGC -- and a state to start from"""
    steps = [2787, 0, OFF, 1 << 31, 1, OFF, 1 << 23]
    target = np.empty(nrows, np.float32)
    floor_bits = np.empty(nrows, np.uint32)
    step = np.empty(nrows, np.uint32)
    state = np.empty(nrows, np.uint32)
    for r in range(nrows):
        target[r], floor_bits[r], _ = agc_np.design(-12.0 - r % 7, 20.0, 40.0 + r % 30, 10_000)
        step[r] = steps[r % len(steps)]
        state[r] = floor_bits[r] if r % 2 == 0 else bits(np.float32(0.37))[0]     # a fresh stream / a carried envelope
    return target, floor_bits, step, state


def _gpu_rows(dev, buf, stride, nrows, n, target, floor_bits, step, state):
    p = dev.upload(buf)
    try:
        new = dev.agc_rows(p, stride, nrows, n, target, floor_bits, step, state)
        out = dev.download(p, buf.size)
    finally:
        dev.free(p)
    return out, new


# ---- 1: wr_agc_rows against the restatement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_rows_against_the_restatement(dev, n, nrows):
    # one row: back to back (16-byte aligned); three rows: an odd stride, so rows that are not aligned; 65 rows: a
    # stride that is a multiple of four frames and larger than the row
    stride = {1: n, 3: n + 5 + n % 2, 65: (n + 3) // 4 * 4 + 4}[nrows]
    v = _rows(nrows, n, seed=1000 * nrows + n)
    target, floor_bits, step, state = _params(nrows)
    buf = np.full(nrows * stride, np.float32(-7.25), np.float32)            # (the gaps between rows must stay as they are)
    for r in range(nrows):
        buf[r * stride: r * stride + n] = v[r]
    out, new = _gpu_rows(dev, buf, stride, nrows, n, target, floor_bits, step, state)
    for r in range(nrows):
        got = out[r * stride: r * stride + n]
        assert np.all(bits(out[r * stride + n: (r + 1) * stride]) == bits(np.float32(-7.25))), r
        if step[r] == OFF:
            assert np.array_equal(bits(got), bits(v[r])), r                  # untouched
            assert new[r] == state[r]
            continue
        want, last = agc_np.apply(v[r], target[r], floor_bits[r], step[r], state[r])
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (r, int(step[r]), bad[:4], got[bad[:4]], want[bad[:4]])
        assert new[r] == last, r
        assert float(np.abs(got).max()) <= float(target[r]) * (1.0 + 2e-7)


def test_a_row_with_an_inf_and_a_nan(dev):
    n = 1500
    v = _rows(1, n, seed=5)[0]
    v[10] = np.inf
    v[500] = np.nan
    v[900] = -np.inf
    target, floor_bits, step = agc_np.design(-12.0, 20.0, 60.0, 10_000)
    out, new = _gpu_rows(dev, v.copy(), n, 1, n, [target], [floor_bits], [step], [floor_bits])
    want, last = agc_np.apply(v, target, floor_bits, step, floor_bits)
    e, _ = agc_np.envelope(v, floor_bits, step, floor_bits)
    assert e[10] == e[500] == e[900] == agc_np.FLT_MAX_BITS               # the rule caps L at FLT_MAX's bits
    nan = np.isnan(want)
    assert nan[500] and np.array_equal(np.isnan(out), nan)
    assert np.array_equal(bits(out)[~nan], bits(want)[~nan])
    assert new[0] == last


# ---- 2: the carry ------------------------------------------------------------------------------------------------------------

def test_one_call_equals_many(dev):
    n = 6000
    v = _rows(1, n, seed=6)[0]
    target, floor_bits, step = agc_np.design(-10.0, 35.0, 50.0, 10_000)
    whole, state_whole = _gpu_rows(dev, v.copy(), n, 1, n, [target], [floor_bits], [step], [floor_bits])
    want, last = agc_np.apply(v, target, floor_bits, step, floor_bits)
    assert np.array_equal(bits(whole), bits(want)) and state_whole[0] == last
    p = dev.upload(v)
    try:
        state, pos = np.array([floor_bits], np.uint32), 0
        for length in (1, 1024, 7, 2500, n - 3532):
            state = dev.agc_rows(p + 4 * pos, length, 1, length, [target], [floor_bits], [step], state)
            pos += length
        assert pos == n
        parts = dev.download(p, n)
    finally:
        dev.free(p)
    assert np.array_equal(bits(parts), bits(whole)) and state[0] == state_whole[0]


# ---- 3: the edge steps ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [700, 2600])
def test_edge_steps(dev, n):
    v = _rows(2, n, seed=7 + n)
    target, floor_bits, _ = agc_np.design(-12.0, 20.0, 60.0, 10_000)
    step = np.array([0, 1 << 31], np.uint32)
    hot = bits(np.float32(3.0e38))[0]                                      # a carried envelope near the top: nothing may wrap
    out, new = _gpu_rows(dev, v.copy().reshape(-1), n, 2, n, [target] * 2, [floor_bits] * 2, step, [floor_bits, hot])
    out = out.reshape(2, n)
    lvl = np.maximum(agc_np.level(v), floor_bits)
    # step 0: the envelope never falls -- it is the running maximum
    want0, last0 = agc_np.apply(v[0], target, floor_bits, 0, floor_bits)
    assert np.array_equal(bits(out[0]), bits(want0)) and new[0] == last0 == int(lvl[0].max())
    # step 2^31: it falls to floor at once -- every frame's envelope is its own level
    want1, last1 = agc_np.apply(v[1], target, floor_bits, 1 << 31, hot)
    assert np.array_equal(bits(out[1]), bits(want1)) and new[1] == last1 == int(lvl[1][-1])
    e1, _ = agc_np.envelope(v[1], floor_bits, 1 << 31, hot)
    assert np.array_equal(e1.astype(np.int64), lvl[1])


# ---- 4, 5: the tuner -----------------------------------------------------------------------------------------------------------

def _agc_settings(c):
    return -12.0 - c % 5, 20.0 * (1 + c % 3), 60.0


def _make(dev, nrx, max_block, nco, agc_on, plain, l2=64, keep=False):
    """nrx receivers, AM / FM / USB / LSB in turn; a squelch on receivers 0 and 7 (the ones _blocks puts carriers on), an
    af_gain on 3 and 4, the sink's scale 32768 -- unless `plain`: scale 1 and gains of 0 dB, whose audio is the rule's v;
    AGC on every third receiver where agc_on"""
    t = Tuner(dev, FS, nrx, max_block, nco)
    chans = [t.add_receiver(f, 128_000, CHAN_RATE, MODES[c % 4], 160, AUDIO_RATE, fir_lengths=(64, l2))
             for c, f in enumerate(_ifs(nrx))]
    if keep:
        t.keep_stages(capi.WR_STAGE_DEMOD)
    for c in (0, 7):
        if c < nrx:
            t.set_squelch(chans[c], -46.0, True)
    if not plain:
        for c, db in ((3, 6.0), (4, -3.5)):
            if c < nrx:
                t.set_af_gain(chans[c], db)
        capi.check(t.lib.wr_tuner_set_audio_scale(t.h, C.c_float(SCALE)))
    if agc_on:
        for c in range(0, nrx, 3):
            t.set_agc(chans[c], *_agc_settings(c))
    return t, chans


def _gain_of(c):
    return {3: np.float32(10.0 ** (6.0 / 20.0)), 4: np.float32(10.0 ** (-3.5 / 20.0))}.get(c, np.float32(1.0))


def _run_twins(dev, nco, k1s, nrx=70, l2=64, keep=False):
    """the three twins over blocks of k1s channel frames; returns the tuners (the caller destroys them) and the last k1"""
    big = max(k1s) * D1
    a, chans = _make(dev, nrx, big, nco, True, False, l2, keep)          # AGC on every third receiver
    b, chans_b = _make(dev, nrx, big, nco, False, False, l2, keep)       # none
    p, chans_p = _make(dev, nrx, big, nco, False, True, l2, keep)        # none, scale 1, gains 0 dB: v
    assert chans == chans_b == chans_p
    par = {c: agc_np.design(*_agc_settings(c), AUDIO_RATE) for c in range(0, nrx, 3)}
    state = {c: par[c][1] for c in par}
    pos, moved = 0, 0
    for blk, k1 in enumerate(k1s):
        n, k2 = k1 * D1, k1 // D2
        iq = _block(n, _ifs(nrx)[::7], seed=40 + blk, pos=pos)
        pos += n
        for t in (a, b, p):
            t.submit_host(iq)
        ga, gb, gp = a.fetch_audio_all(), b.fetch_audio_all(), p.fetch_audio_all()
        assert ga.shape == gb.shape == gp.shape == ((nrx + 63) // 64 * 64, k2)
        for c, ch in enumerate(chans):
            s = a.slot(ch)
            assert s == b.slot(ch) == p.slot(ch)
            if c not in par:
                assert np.array_equal(bits(ga[s]), bits(gb[s])), (blk, c)     # as if there were no AGC anywhere
                continue
            v = gp[s]
            assert not np.any((v != 0) & (np.abs(v) < TINY))
            target, floor_bits, step = par[c]
            want, state[c] = agc_np.apply(v, target, floor_bits, step, state[c], _gain_of(c), SCALE)
            bad = np.flatnonzero(bits(ga[s]) != bits(want))
            assert bad.size == 0, (blk, c, bad[:4], ga[s][bad[:4]], want[bad[:4]])
            moved += int(np.count_nonzero(bits(ga[s]) != bits(gb[s])))
        # the squelch mutes, and the AGC leaves a muted frame muted
        assert np.any(gp[a.slot(chans[0])] == 0.0) and np.any(gp[a.slot(chans[0])] != 0.0)
    assert moved > 0                                                      # the AGC did something
    for c, ch in enumerate(chans):
        on, target, floor_bits, step, st = a.get_agc(ch)
        if c in par:
            assert (on, bits(target)[0], floor_bits, step, st) == (True, bits(par[c][0])[0], par[c][1], par[c][2], state[c]), c
        else:
            assert (on, floor_bits, step, st) == (False, 0, 0, 0)
    assert a.agc_info() == (len(par), len(k1s))                           # one launch per block of the one rate group
    assert b.agc_info() == (0, 0) and p.agc_info() == (0, 0)
    return (a, b, p), chans


def _destroy(tuners):
    for t in tuners:
        t.destroy()


@pytest.mark.parametrize("nco", [capi.WR_NCO_EXACT, capi.WR_NCO_ROTATE], ids=["exact", "rotate"])
def test_tuner(dev, nco):
    """two lane groups, 70 receivers, three blocks of different lengths, the second shorter than the filter history"""
    tuners, _ = _run_twins(dev, nco, [600, 40, 257])
    _destroy(tuners)


def test_the_two_kernel_path(dev):
    """keep_stages(DEMOD): k_tuner_demod + k_tuner_audio; the demodulator rows are what they were"""
    k1s = [257, 120]
    (a, b, p), chans = _run_twins(dev, capi.WR_NCO_EXACT, k1s, keep=True)
    for ch in chans[::3][:8] + chans[1::9]:
        da, db = a.fetch(ch, capi.WR_STAGE_DEMOD, k1s[-1]), b.fetch(ch, capi.WR_STAGE_DEMOD, k1s[-1])
        assert da.size == k1s[-1] and np.array_equal(bits(da), bits(db))
    _destroy((a, b, p))


def test_a_long_audio_filter(dev):
    """a 128-tap audio filter: k_tuner_post<D2, 2>"""
    tuners, _ = _run_twins(dev, capi.WR_NCO_ROTATE, [257, 100], l2=128)
    _destroy(tuners)


# ---- 6: what sets the state to floor, and what keeps it -----------------------------------------------------------------------

def test_state_resets(dev):
    k1, nrx = 120, 4
    n, k2 = k1 * D1, k1 // D2
    a, chans = _make(dev, nrx, n, capi.WR_NCO_EXACT, False, True)
    p, _ = _make(dev, nrx, n, capi.WR_NCO_EXACT, False, True)
    sets = {0: (-12.0, 20.0, 60.0), 1: (-6.0, 5.0, 40.0)}
    for c, s in sets.items():
        a.set_agc(chans[c], *s)
    state = {}
    pos = [0]

    def block(reset=()):
        """one block through both; receivers in `reset` must start from floor, the others from where they were"""
        iq = _block(n, _ifs(nrx)[::7], seed=60 + pos[0] // n, pos=pos[0])
        pos[0] += n
        a.submit_host(iq)
        p.submit_host(iq)
        ga, gp = a.fetch_audio_all(), p.fetch_audio_all()
        for c, s in sets.items():
            target, floor_bits, step = agc_np.design(*s, AUDIO_RATE)
            if c in reset or c not in state:
                state[c] = floor_bits
            else:
                assert state[c] > floor_bits                                # (carried: the case says something)
            want, state[c] = agc_np.apply(gp[a.slot(chans[c])], target, floor_bits, step, state[c])
            assert np.array_equal(bits(ga[a.slot(chans[c])]), bits(want)), (pos[0] // n, c)
            assert a.get_agc(chans[c])[4] == state[c]
        for c in range(nrx):
            if c not in sets:
                assert np.array_equal(bits(ga[a.slot(chans[c])]), bits(gp[a.slot(chans[c])]))

    block()
    for t in (a, p):                                                        # (the filters' histories go too: on both)
        capi.check(t.lib.wr_chan_reset_history(t.h, chans[0]))
    block(reset=(0,))
    sets[1] = (-20.0, 60.0, 30.0)                                           # new settings keep the state
    a.set_agc(chans[1], *sets[1])
    block()
    a.set_agc(chans[0], enable=False)                                       # off and on again
    a.set_agc(chans[0], *sets[0])
    block(reset=(0,))
    for t in (a, p):
        t.seek(pos[0])
    block(reset=(0, 1))
    a.set_agc(chans[1], enable=False)                                       # off: the receiver's bits are the twin's again
    del sets[1]
    block()
    assert a.get_agc(chans[1])[0] is False and a.agc_info()[0] == 1
    _destroy((a, p))


# ---- 7: the ring and the getters see the same block -----------------------------------------------------------------------------

def test_ring_and_getters(dev):
    k1, nrx = 257, 6
    n, k2 = k1 * D1, k1 // D2
    a, chans = _make(dev, nrx, n, capi.WR_NCO_ROTATE, True, False)
    b, _ = _make(dev, nrx, n, capi.WR_NCO_ROTATE, False, False)
    a.audio_ring(4)
    seen = []
    for blk in range(2):
        iq = _block(n, _ifs(nrx)[::7], seed=70 + blk, pos=blk * n)
        seq = a.submit_count()
        a.submit_host(iq)
        b.submit_host(iq)
        ga = a.fetch_audio_all()
        for ch in chans:
            assert np.array_equal(bits(a.fetch(ch, capi.WR_STAGE_AUDIO, k2)), bits(ga[a.slot(ch)]))
        p_dev, stride, frames = a.audio_dev()
        assert frames == k2
        assert np.array_equal(bits(dev.download(p_dev + 4 * stride * a.slot(chans[3]), k2)), bits(ga[a.slot(chans[3])]))
        seen.append((seq, ga))
        assert not np.array_equal(bits(ga[a.slot(chans[0])]), bits(b.fetch_audio_all()[b.slot(chans[0])]))
    for seq, ga in seen:
        rows, got_seq = a.ring_acquire()
        assert got_seq == seq and rows.shape == ga.shape
        assert np.array_equal(bits(rows), bits(ga))
        a.ring_release()
    assert a.ring_stats() == (0, 0)
    _destroy((a, b))


# ---- 8: streaming ---------------------------------------------------------------------------------------------------------------

def test_streaming_waits_for_the_agc_to_go_off(dev):
    k1, nrx, nblk = 65, 4, 4
    n, k2 = k1 * D1, k1 // D2
    iq = _block(nblk * n, _ifs(nrx)[::7], seed=80)
    x = dev.upload(iq)
    tuners = []
    try:
        a, chans = _make(dev, nrx, n, capi.WR_NCO_ROTATE, False, True)
        b, _ = _make(dev, nrx, n, capi.WR_NCO_ROTATE, False, True)
        tuners = [a, b]
        for t in tuners:
            t.audio_ring(nblk)
            t.streaming(True)
        a.set_agc(chans[1], -12.0, 20.0, 60.0)
        live = []
        for blk in range(nblk):
            if blk == 2:
                a.set_agc(chans[1], enable=False)
            a.submit_device(x + 8 * n * blk, n)
            live.append(a.stream_info()[0])
        assert live == [False, False, True, True]                           # no launch is open while the AGC is on
        for blk in range(nblk):
            b.submit_device(x + 8 * n * blk, n)
        assert b.stream_info()[0] is True
        assert a.agc_info()[1] == 2
        target, floor_bits, step = agc_np.design(-12.0, 20.0, 60.0, AUDIO_RATE)
        state = floor_bits
        for blk in range(nblk):
            ra, sa = a.ring_acquire()
            rb, sb = b.ring_acquire()
            assert sa == sb == blk and ra.shape == rb.shape == (64, k2)
            for c, ch in enumerate(chans):
                s = a.slot(ch)
                if c == 1 and blk < 2:
                    want, state = agc_np.apply(rb[s], target, floor_bits, step, state)
                    assert np.array_equal(bits(ra[s]), bits(want)), blk
                    assert not np.array_equal(bits(ra[s]), bits(rb[s]))
                else:
                    assert np.array_equal(bits(ra[s]), bits(rb[s])), (blk, c)
            a.ring_release()
            b.ring_release()
        assert a.stream_info()[1] >= 1 and a.stream_info()[2] == 2          # blocks 2 and 3 were streamed
    finally:
        _destroy(tuners)
        dev.free(x)
