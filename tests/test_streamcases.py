"""Without a GPU: the comparisons of tests/streamcases.py that the streaming launch's GPU tests rely on.  The probe selectors
cover what those tests say they cover, for every receiver count and layout they run; against_oracle accepts the oracle's own
output and rejects each single fault at twice its bound; bits() and same_bits() are comparisons of bits."""
import copy

import numpy as np
import pytest

import streamcases as sc
from tunercases import AUDIO_ATOL, IQ_ATOL, LINEAR_ATOL, bits, bits_f32
from webradio_amd import capi, synth


# ---- the probe selectors cover what the GPU tests assert ----------------------------------------------------------------------------

def _slots(nch):
    return dict(slots=list(range(nch)))


COUNTS = sorted(set(sc.LANE_CASES.values()) | {case[3] for case in sc.BLOCK_EDGE_CASES.values()})


@pytest.mark.parametrize("nch", COUNTS)
def test_probes_reach_every_lane_group_and_demodulator(nch):
    chosen = sc.probes(nch)
    assert all(0 <= c < nch for c in chosen) and set(sc.fm_probes(nch)) <= set(chosen)
    assert all(c % 4 == 0 for c in sc.fm_probes(nch))                     # MODES[0] is FM: the carriers sit on FM receivers
    sc.covers_groups_and_modes(nch)(_slots(nch), chosen)
    with pytest.raises(AssertionError, match="lane groups"):
        sc.covers_groups_and_modes(nch + 64)(_slots(nch + 64), chosen)
    with pytest.raises(AssertionError, match="demodulators"):
        sc.covers_groups_and_modes(nch)(_slots(nch), [c - c % 4 for c in chosen])     # every lane group still, FM alone


LONG_COUNTS = sorted(set(sc.LANE_CASES.values()) | {c[1] for cases in sc.LONG_MIXED_FILTERS.values() for c in cases})


@pytest.mark.parametrize("nch", LONG_COUNTS)
def test_group_probes_reach_every_demodulator_in_every_lane_group(nch):
    chosen = sc.group_probes(nch)
    assert set(sc.probes(nch)) <= set(chosen) and all(0 <= c < nch for c in chosen)
    sc.covers_modes_in_groups(nch)(_slots(nch), chosen)
    with pytest.raises(AssertionError, match="leave out"):
        sc.covers_modes_in_groups(nch)(_slots(nch), sc.probes(nch))
    with pytest.raises(AssertionError, match="slot"):
        sc.covers_modes_in_groups(nch)(dict(slots=list(range(nch))[::-1]), chosen)


LAYOUTS = ([("per-group-%d" % n, sc.per_group(n)) for n in sc.FILTER_PER_GROUP_COUNTS]
           + [("PD2=%d" % p, (sc.spread if lay == "spread" else sc.staggered)(n, k)) for p, (n, k, lay, _) in sorted(sc.MIXED_FILTERS.items())]
           + [("L2=%d-PD2=%d" % (l2, p), (sc.spread if lay == "spread" else sc.staggered)(n, k))
              for l2, cases in sorted(sc.LONG_MIXED_FILTERS.items()) for p, n, k, lay in cases]
           + [("four-of-130", sc.spread(130, 4)), ("five-of-70", sc.spread(70, 5))])


@pytest.mark.parametrize("bins", [b for _, b in LAYOUTS], ids=[i for i, _ in LAYOUTS])
def test_passband_probes_reach_every_distinct_passband(bins):
    nch = len(bins)
    chosen = sc.passband_probes(bins)
    sc.covers_passbands(bins)(_slots(nch), chosen)
    assert set(sc.fm_probes(nch)) <= set(chosen)
    linear = [c for c in chosen if c % 4 != 0]
    one_missing = [c for c in chosen if bins[c] != bins[linear[0]]]
    with pytest.raises(AssertionError, match="passbands"):
        sc.covers_passbands(bins)(_slots(nch), one_missing)
    assert not set(sc.passband_probes(bins, skip=(linear[0],))) & {linear[0]}


# ---- against_oracle accepts the oracle and rejects a single fault -----------------------------------------------------------------

NCH, PD2, NBLK, K2 = 70, 5, 2, 100            # the smallest case of the stream tests: two blocks of 100 audio frames


def _case(oracle, which, silent=False):
    """(yardstick, host blocks, probes, a run made of the oracle's own outputs) for 70 receivers at DECIMATION_RATES[5]"""
    fs, crate = sc.DECIMATION_RATES[PD2]
    arate, n = crate // PD2, K2 * PD2 * (fs // crate)
    ifs = sc.spread_ifs(fs, NCH)
    if silent:      # no carrier and no noise either: on noise alone the FM detector is as loud as on a carrier
        iq = np.zeros(2 * NBLK * n, np.float32)
    else:
        iq = synth.fm_stream(NBLK * n, fs, sc.carriers(ifs), amp=0.1)
    blocks = [iq[2 * n * b: 2 * n * (b + 1)] for b in range(NBLK)]
    if which == "receivers":
        yardstick, chosen = sc.ProbeOracle(oracle, fs, crate, arate, ifs), sc.probes(NCH)
    else:
        yardstick, chosen = sc.ProbeOracle(oracle, fs, crate, arate, ifs, 128), sc.group_probes(NCH)
    audio = [np.zeros((NCH, K2), np.float32) for _ in range(NBLK)]
    chan = [np.zeros(2 * K2 * PD2, np.float32) for _ in range(NCH)]
    for c in chosen:
        rx = yardstick.rx(c)
        for b, blk in enumerate(blocks):
            wa, wc, _ = rx.run(blk)
            audio[b][c], chan[c] = wa, wc.copy()
    run = dict(got=[(b, a) for b, a in enumerate(audio)], slots=list(range(NCH)), iq=chan)
    return yardstick, blocks, chosen, run


@pytest.fixture(scope="module", params=["receivers", "chains"])
def case(request, oracle):
    return _case(oracle, request.param)


def _tolerance(yardstick, c):
    gain2 = max(1.0, float(np.abs(yardstick.audio_taps(c)).sum()))
    return AUDIO_ATOL * gain2 if c % 4 == 0 else yardstick.tol_linear(gain2)


def test_the_oracles_own_output_is_accepted(case):
    yardstick, blocks, chosen, run = case
    sc.against_oracle(yardstick, blocks, run, chosen, sc.covers_groups_and_modes(NCH))
    # the bounds are the ones the docstrings state
    linear = next(c for c in chosen if c % 4 != 0)
    gain2 = max(1.0, float(np.abs(yardstick.audio_taps(linear)).sum()))
    assert yardstick.tol_linear(gain2) == (AUDIO_ATOL if yardstick.l2 is None else LINEAR_ATOL * gain2)
    assert sc.MODES[0] == capi.WR_FM and _tolerance(yardstick, 0) == AUDIO_ATOL * gain2


@pytest.mark.parametrize("fm", [False, True], ids=["linear", "fm"])
def test_an_audio_sample_off_by_twice_its_bound_is_rejected(case, fm):
    yardstick, blocks, chosen, run = case
    c = next(c for c in chosen if (c % 4 == 0) == fm and c > 0)
    tol = _tolerance(yardstick, c)
    near, far = copy.deepcopy(run), copy.deepcopy(run)
    near["got"][1][1][c, 37] += np.float32(0.5 * tol)
    far["got"][1][1][c, 37] += np.float32(2.0 * tol)
    sc.against_oracle(yardstick, blocks, near, chosen)
    with pytest.raises(AssertionError, match=r"receiver %d \(mode %d\), block 1: audio off by" % (c, sc.MODES[c % 4])):
        sc.against_oracle(yardstick, blocks, far, chosen)
    sc.against_oracle(yardstick, blocks, far, chosen, check_blocks={0})   # ... where that block is looked at


def test_a_channel_iq_sample_off_by_twice_its_bound_is_rejected(case):
    yardstick, blocks, chosen, run = case
    c = chosen[-1]
    near, far = copy.deepcopy(run), copy.deepcopy(run)
    near["iq"][c][11] += np.float32(0.5 * IQ_ATOL)
    far["iq"][c][11] += np.float32(2.0 * IQ_ATOL)
    sc.against_oracle(yardstick, blocks, near, chosen)
    with pytest.raises(AssertionError, match="receiver %d: last block's channel IQ off by" % c):
        sc.against_oracle(yardstick, blocks, far, chosen)


def test_a_wrong_shape_is_reported_as_one(case):
    yardstick, blocks, chosen, run = case
    short = copy.deepcopy(run)
    short["got"][0] = (0, short["got"][0][1][:, :-1])
    with pytest.raises(AssertionError, match=r"block 0: audio of shape \(99,\), the oracle's \(100,\)"):
        sc.against_oracle(yardstick, blocks, short, chosen)
    short = copy.deepcopy(run)
    short["iq"][chosen[0]] = short["iq"][chosen[0]][:-2]
    with pytest.raises(AssertionError, match="channel IQ of shape"):
        sc.against_oracle(yardstick, blocks, short, chosen)


def test_a_probe_set_that_misses_its_coverage_is_rejected_first(case):
    yardstick, blocks, chosen, run = case
    with pytest.raises(AssertionError, match="lane groups"):
        sc.against_oracle(yardstick, blocks, run, [c for c in chosen if c < 64], sc.covers_groups_and_modes(NCH))


@pytest.mark.parametrize("which", ["receivers", "chains"])
def test_a_stream_without_a_carrier_is_rejected(oracle, which):
    yardstick, blocks, chosen, run = _case(oracle, which, silent=True)
    with pytest.raises(AssertionError, match="no carrier was heard"):
        sc.against_oracle(yardstick, blocks, run, chosen, sc.covers_groups_and_modes(NCH))


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------

def test_bits_tell_signed_zeros_and_nan_payloads_apart():
    zeros = np.array([0.0, -0.0], np.float32)
    assert zeros[0] == zeros[1] and bits(zeros)[0] != bits(zeros)[1]
    assert bits_f32([0.0])[0] != bits_f32([-0.0])[0] and bits_f32(-0.0).tolist() == [0x80000000]
    nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000], np.uint32).view(np.float32)
    assert np.isnan(nans).all()
    for view in (bits, bits_f32):
        assert len(set(view(nans).tolist())) == 3 and np.array_equal(view(nans), view(nans.copy()))
    assert bits(nans[::2]).tolist() == [0x7FC00000, 0xFFC00000]         # a strided view: its own elements
    assert bits_f32(np.array([1.5], np.float64)).tolist() == [0x3FC00000] and bits(np.array([1.5], np.float32)).tolist() == [0x3FC00000]


NAN_A, NAN_B = 0x7FC00000, 0x7FC00001


def _word(a, at, word):
    a.view(np.uint32)[at] = word


def test_same_bits_is_a_comparison_of_bits():
    audio = np.array([[0.25, 0.0, 0.0], [1.0, -0.0, 2.0]], np.float32)
    chan = np.array([0.5, -0.5, 0.0, 0.0], np.float32)
    _word(audio, (0, 2), NAN_A)
    _word(chan, 3, NAN_A)
    one = dict(got=[(0, audio)], slots=[0, 1], iq=[chan, chan.copy()], state=[(123, (0.0, 0.125)), (456, (0.0, 0.125))])
    assert np.isnan(audio[0, 2]) and np.isnan(chan[3])
    sc.same_bits(one, copy.deepcopy(one))                                 # NaNs included: equal bits are equal
    for what, change in (("audio samples differ", lambda r: r["got"][0][1].__setitem__((0, 1), np.float32(-0.0))),
                         ("audio samples differ", lambda r: _word(r["got"][0][1], (0, 2), NAN_B)),
                         ("channel-IQ floats", lambda r: r["iq"][1].__setitem__(2, np.float32(-0.0))),
                         ("channel-IQ floats", lambda r: _word(r["iq"][0], 3, NAN_B)),
                         ("previous frame", lambda r: r["state"].__setitem__(1, (456, (-0.0, 0.125)))),
                         ("NCO phase", lambda r: r["state"].__setitem__(0, (124, (0.0, 0.125)))),
                         ("sequence numbers", lambda r: r["got"].__setitem__(0, (1, r["got"][0][1]))),
                         ("audio of shape", lambda r: r["got"].__setitem__(0, (0, r["got"][0][1][:, :2])))):
        other = copy.deepcopy(one)
        change(other)
        with pytest.raises(AssertionError, match=what):
            sc.same_bits(one, other)
