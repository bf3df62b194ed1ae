"""-m gpu: the streaming launch (k_tuner_stream) for tuners whose receivers have an audio filter of 128 or 256 taps.

LowPass::_firLength is a run-time value (dsp/lowpass.cxx:38-39); the tuner builds a 128- or 256-tap audio filter as 2 or 4
segments of 64 taps (post_role<D2, false, NSEG>), which tests/test_gpu_f4.py holds to the oracle on the launch-per-block
path.  k_tuner_stream<PD2, NG, TS, NSEG> takes such a tuner too: 128 taps at every audio decimation the launch has,
256 taps up to an audio decimation of 3 (beyond it the post stage's window leaves a CU room for one workgroup and the
tuner keeps its launch per block: DESIGN.md 3.6).  A block must hold L2 channel-rate frames at least: L2 - 1 rows of
history for the block behind it and the frame in front of them.

Every case asserts the exact stream_info() tuple (a silent fall-back to a launch per block fails), the SAME BITS as one
launch per block on a fresh tuner (every block's audio on every receiver, the last block's channel IQ, every receiver's
state), and holds probe receivers of all four demodulators in every lane group to the oracle's chain with an L2-tap audio
filter (tunercases.OracleChain), within tunercases' ROTATE bounds: channel IQ IQ_ATOL; audio LINEAR_ATOL x sum|h2| for AM,
USB and LSB (|.| and the Re / Im sums are 2-Lipschitz in the channel IQ, then the linear filter), AUDIO_ATOL x sum|h2| for
FM as the stream tests have it (streamcases.ProbeOracle)."""
import numpy as np
import pytest

import launch_plan
import streamcases as sc
from streamcases import DECIMATION_RATES, LANE_CASES, pb, sets_per_group, spread, staggered
from webradio_amd import capi

pytestmark = pytest.mark.gpu

# the audio decimations a launch must take, by audio filter length (wr_stream_kernel.inc: with_stream_nseg)
STREAMED_D2 = {128: sorted(DECIMATION_RATES), 256: [1, 2, 3]}


def _k2_for(l2, d2, k2=100):
    """about 100 audio frames a block -- more where the block would otherwise hold fewer than L2 channel-rate frames"""
    return max(k2, -(-l2 // d2) + 5)


def _play_long(dev, fs, crate, arate, ifs, l2, blocks, stream, submit, **more):
    """streamcases.play with an audio filter of l2 taps on every receiver"""
    return sc.play(dev, fs, crate, arate, ifs, blocks, stream, submit, fir_lengths=(64, l2), **more)


def _stream_vs_blocks(dev, oracle, l2, fs, crate, arate, nch, n, nblk, expect, u8=False):
    """streamcases.stream_vs_blocks with an audio filter of l2 taps on every receiver: every demodulator is probed in every
    lane group (streamcases.group_probes) against the oracle's chain"""
    ifs = sc.spread_ifs(fs, nch)
    return sc.stream_vs_blocks(dev, sc.ProbeOracle(oracle, fs, crate, arate, ifs, l2), fs, crate, arate, ifs, n, nblk, expect,
                               sc.group_probes(nch), sc.covers_modes_in_groups(nch), u8=u8, fir_lengths=(64, l2))


INSTANCES = [(l2, pd2, lanes) for l2 in sorted(STREAMED_D2) for pd2 in STREAMED_D2[l2] for lanes in LANE_CASES]


@pytest.mark.parametrize("l2,pd2,lanes", INSTANCES, ids=[f"L2={a}-PD2={p}-{l}" for a, p, l in INSTANCES])
def test_long_audio_filter_streams_at_every_instance(dev, oracle, l2, pd2, lanes):
    """k_tuner_stream<PD2, NG, 1, L2 / 64> for NG in {1, 2}: 128 taps at every audio decimation the launch has, 256 taps at
    1, 2 and 3 -- five blocks of about 100 audio frames through ONE launch, 2 and 3 lane groups with a ragged last"""
    fs, crate = DECIMATION_RATES[pd2]
    nch = LANE_CASES[lanes]
    d1 = fs // crate
    k2 = _k2_for(l2, pd2)
    assert k2 * pd2 >= l2
    _stream_vs_blocks(dev, oracle, l2, fs, crate, crate // pd2, nch, k2 * pd2 * d1, 5, (True, 1, 5))


def test_256_taps_at_an_audio_decimation_of_5(dev, oracle):
    """256 taps from an audio decimation of 4 on: the post stage's window (89 KB at D2 = 5) leaves a CU's LDS room for one
    workgroup.  Such a tuner either streams (a launch built with a narrower tile) or keeps its launch per block --
    nothing in between -- and gives the same bits and the oracle's audio either way."""
    fs, crate = DECIMATION_RATES[5]
    nblk = 4
    _stream_vs_blocks(dev, oracle, 256, fs, crate, crate // 5, 130, 100 * 5 * (fs // crate), nblk,
                      {(True, 1, nblk), (False, 0, 0)})


# id: (audio taps, audio decimation, audio frames per block, does it stream)
EDGE_CASES = {
    "L2=128-smallest": (128, 5, 26, True),                # k1 = 130: the smallest multiple of D2 that is >= L2
    "L2=128-below": (128, 5, 25, False),                  # k1 = 125: the largest below it
    "L2=256-smallest": (256, 3, 86, True),                # k1 = 258
    "L2=256-below": (256, 3, 85, False),                  # k1 = 255
    "L2=256-exactly": (256, 1, 256, True),                # k1 = L2: sixteen whole tiles, the history is the whole block before
    "L2=256-one-short": (256, 1, 255, False),
    "L2=128-one-tile-exactly": (128, 8, 16, True),        # k1 = L2 = 128 and ONE tile of 16 audio frames
    "L2=128-one-tile": (128, 10, 16, True),               # k1 = 160: one tile
    "L2=128-ragged-tile": (128, 5, 57, True),             # 3 tiles and 9 frames
    "L2=256-ragged-tile": (256, 2, 135, True),            # 8 tiles and 7 frames
}


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_long_audio_filter_block_edges(dev, oracle, case):
    """A block streams from L2 channel-rate frames on (L2 - 1 rows of history for the block behind it and the frame in
    front of them) -- the smallest multiple of D2 that is, and the largest that is not, which takes a launch per block and
    gives the right bits; a ragged last tile; a block of one tile."""
    l2, pd2, k2, streams = EDGE_CASES[case]
    fs, crate = DECIMATION_RATES[pd2]
    k1 = k2 * pd2
    assert (k1 >= l2) == streams
    if "smallest" in case or "exactly" in case:
        assert k1 - pd2 < l2 <= k1
    if "below" in case or "one-short" in case:
        assert k1 < l2 <= k1 + pd2
    if "ragged" in case:
        assert k2 > launch_plan.post_tk() and k2 % launch_plan.post_tk()
    if "one-tile" in case:
        assert k2 == launch_plan.post_tk()
    nblk = 4
    _stream_vs_blocks(dev, oracle, l2, fs, crate, crate // pd2, 70, k1 * (fs // crate), nblk,
                      (True, 1, nblk) if streams else (False, 0, 0))


@pytest.mark.parametrize("l2,pd2", [(128, 5), (256, 3)])
def test_long_audio_filter_state_goes_both_ways(dev, oracle, l2, pd2):
    """One tuner: two blocks with a launch each, flush(), two blocks streamed, flush(), one block with a launch of its own --
    against five blocks with a launch each.  The stream's block 0 takes its L2 - 1 rows of history from the tuner's state
    (dem_hist), its second block from the channel-IQ ring (chan_prev), and the closing state task leaves L2 - 1 rows and
    the last channel frame for the launch behind it."""
    fs, crate = DECIMATION_RATES[pd2]
    arate, nch, nblk = crate // pd2, 130, 5
    n = _k2_for(l2, pd2, 60) * pd2 * (fs // crate)
    ifs = sc.spread_ifs(fs, nch)
    host_blocks, blocks, submit = sc.device_stream(fs, ifs, n, nblk)
    seen = {}

    def phases(t, b):
        if b in (2, 4):
            if b == 4:
                seen["streamed"] = t.stream_info()
            t.flush()
            t.streaming(b == 2)

    one = _play_long(dev, fs, crate, arate, ifs, l2, blocks, False, submit)
    many = _play_long(dev, fs, crate, arate, ifs, l2, blocks, phases, submit)
    assert one["info"] == (False, 0, 0)
    assert seen["streamed"] == (True, 1, 2), seen
    assert many["info"] == (False, 1, 2), many["info"]
    sc.same_bits(one, many)
    sc.against_oracle(sc.ProbeOracle(oracle, fs, crate, arate, ifs, l2), host_blocks, many,
                      sc.group_probes(nch), sc.covers_modes_in_groups(nch))


@pytest.mark.parametrize("l2,pd2", [(128, 5), (256, 2)])
def test_an_audio_passband_per_receiver_and_setters_between_blocks(dev, oracle, l2, pd2):
    """Half of lane group 0 has an audio passband of its own: that group's taps come per lane (WrPostArgs::uni2 clear),
    lane groups 1 and 2 share one filter each and read it through the scalar cache (uni2 set).  A retune and a change of
    mode between blocks close the launch at their block boundary, and the next block opens another -- the counts of
    test_gpu_stream_filters.test_filter_setters_mid_stream."""
    fs, crate = DECIMATION_RATES[pd2]
    arate, nch, nblk = crate // pd2, 130, 6
    n = _k2_for(l2, pd2, 60) * pd2 * (fs // crate)
    ifs = sc.spread_ifs(fs, nch)
    _, apb = sc.passbands(fs, crate, arate)
    apbs = [apb // 2 if c < 32 else apb for c in range(nch)]
    assert oracle.lowpass_maxbin_n(l2, apb // 2, crate) >= 1
    assert not np.array_equal(oracle.lowpass_design(apb // 2, crate, l2), oracle.lowpass_design(apb, crate, l2))
    retuned, remoded = 70, 9                     # lane group 1 (shared filter) and lane group 0 (per-lane taps)
    host_blocks, blocks, submit = sc.device_stream(fs, ifs, n, nblk)

    def run(stream):
        seen = {}

        def between(t, chans, b):
            if b in (2, 4):
                seen[b] = t.stream_info()
                if b == 2:
                    t.set_if(chans[retuned], ifs[retuned] + 777)
                else:
                    t.set_mode(chans[remoded], capi.WR_AM)
            return []

        return _play_long(dev, fs, crate, arate, ifs, l2, blocks, stream, submit, between=between, apbs=apbs), seen

    one, seen1 = run(False)
    many, seen = run(True)
    assert one["info"] == (False, 0, 0) and all(v == (False, 0, 0) for v in seen1.values())
    assert seen[2] == (True, 1, 2), seen            # blocks 0, 1: one launch
    assert seen[4] == (True, 2, 4), seen            # blocks 2, 3: the retune closed it, block 2 opened the second
    assert many["info"] == (True, 3, 6), many["info"]   # blocks 4, 5: behind the change of mode, a third
    sc.same_bits(one, many)
    probes = [c for c in sc.group_probes(nch) if c not in (retuned, remoded)]
    assert {apbs[c] for c in probes} == {apb // 2, apb}
    # (no coverage condition beyond the one above: the two receivers left out were their lane group's probes of a demodulator)
    sc.against_oracle(sc.ProbeOracle(oracle, fs, crate, arate, ifs, l2, apbs=apbs),
                      host_blocks, many, probes)


def test_long_audio_filter_streams_byte_blocks(dev, oracle):
    """the RTL-SDR byte format (io/rtlsdrtuner.cxx:106) out of device memory, 128 taps at D2 = 8 (BASELINE config 1's
    decimations)"""
    fs, crate = DECIMATION_RATES[8]
    _stream_vs_blocks(dev, oracle, 128, fs, crate, crate // 8, 70, 100 * 8 * (fs // crate), 4, (True, 1, 4), u8=True)


MIXED_CASES = [(l2,) + c for l2 in sorted(sc.LONG_MIXED_FILTERS) for c in sc.LONG_MIXED_FILTERS[l2]]


@pytest.mark.parametrize("l2,pd2,nch,k,layout", MIXED_CASES, ids=[f"L2={c[0]}-PD2={c[1]}-{c[3]}-filters" for c in MIXED_CASES])
def test_long_audio_filter_with_channel_passbands_per_receiver(dev, oracle, l2, pd2, nch, k, layout):
    """k_tuner_stream<PD2, 1, WR_TAPSETS, L2 / 64>: 2, 3 and 4 distinct channel passbands across the lanes of a lane group
    (receiverhandler.cxx:130-137; tests/test_gpu_stream_filters.py's layouts) on a tuner whose audio filters have 128 or
    256 taps -- a window copy per channel filter in the DDC waves, the long window in the post stage.  One launch, the
    bits of a launch per block, every distinct channel passband probed against the oracle's chain."""
    fs, crate = DECIMATION_RATES[pd2]
    arate, nblk = crate // pd2, 4
    bins = (spread if layout == "spread" else staggered)(nch, k)
    sets = sets_per_group(bins)
    assert max(sets) == k > 1 and (layout == "spread" or len(set(sets)) > 1), sets
    cpbs = [pb(fs, m) for m in bins]
    n = _k2_for(l2, pd2, 60) * pd2 * (fs // crate)
    ifs = sc.spread_ifs(fs, nch)
    host_blocks, blocks, submit = sc.device_stream(fs, ifs, n, nblk)

    one = _play_long(dev, fs, crate, arate, ifs, l2, blocks, False, submit, cpbs=cpbs)
    many = _play_long(dev, fs, crate, arate, ifs, l2, blocks, True, submit, cpbs=cpbs)
    assert one["info"] == (False, 0, 0)
    assert many["info"] == (True, 1, nblk), many["info"]
    sc.same_bits(one, many)
    probes = sc.group_probes(nch)
    for m in sorted(set(bins)):                        # every distinct channel passband, by a linear demodulator too
        probes += [c for c in range(nch) if bins[c] == m and c % 4 != 0][:1]
    probes = sorted(set(probes))
    assert {bins[c] for c in probes} == set(bins)
    sc.against_oracle(sc.ProbeOracle(oracle, fs, crate, arate, ifs, l2, cpbs=cpbs),
                      host_blocks, many, probes, sc.covers_modes_in_groups(nch))
