"""-m gpu: the streaming launch (k_tuner_stream) for tuners whose receivers have channel passbands of their own.

The reference gives every receiver its own passband control (receiverhandler.cxx:130-137 -> LowPass::setPassband,
lowpass.cxx:55-61); radio.cxx:78-82 only sets defaults.  A tuner streams as long as every lane group of 64 channels holds
at most WR_TAPSETS (4) distinct 64-tap channel filters -- k_tuner_stream<PD2, 1, WR_TAPSETS> keeps one window copy per
filter, as k_tuner_ddc does.  Every case holds the streamed run to the SAME BITS as one launch per block (every block's
audio, the last block's channel IQ, every receiver's state), asserts the exact stream_info() counts (a silent fall-back to
a launch per block fails), and holds probe receivers of every distinct passband to oracle.Receiver built with that
receiver's own passband."""
import numpy as np
import pytest

import streamcases as sc
from streamcases import DECIMATION_RATES, pb, per_group, sets_per_group, spread, staggered
from tunercases import AUDIO_ATOL, IQ_ATOL, drain
from webradio_amd import capi, synth
from webradio_amd.device import Tuner

pytestmark = pytest.mark.gpu


def _setter(fs, crate, bins):
    """streamcases.play's `between`: before block 0, every receiver's channel passband (Receiver::channelFilter()->setPassband)"""
    def between(t, chans, b):
        if b == 0:
            for c, ch in enumerate(chans):
                t.set_filter(ch, 0, pb(fs, bins[c]), crate)
        return []
    return between


def _yardstick(oracle, fs, crate, arate, ifs, bins):
    """oracle.Receiver with the probe's OWN channel passband, within streamcases' tolerances"""
    return sc.ProbeOracle(oracle, fs, crate, arate, ifs, cpbs=[pb(fs, m) for m in bins])


def _stream_vs_blocks(dev, oracle, fs, crate, arate, bins, n, nblk, expect, u8=False):
    """streamcases.stream_vs_blocks with a channel passband per receiver, set before block 0: the exact stream_info()
    `expect` = (launches, blocks); every distinct passband is probed (streamcases.passband_probes)"""
    launches, taken = expect
    ifs = sc.spread_ifs(fs, len(bins))
    return sc.stream_vs_blocks(dev, _yardstick(oracle, fs, crate, arate, ifs, bins), fs, crate, arate, ifs, n, nblk,
                               (launches > 0, launches, taken), sc.passband_probes(bins), sc.covers_passbands(bins), u8=u8,
                               between=_setter(fs, crate, bins))


FS, CRATE, ARATE = 2_400_000, 240_000, 48_000         # D1 = 10, D2 = 5
N = 100 * 5 * 10                                      # 100 audio frames a block


@pytest.mark.parametrize("nch", sc.FILTER_PER_GROUP_COUNTS, ids=lambda n: f"{sc.lane_groups(n)}-groups")
def test_a_filter_per_lane_group_streams(dev, oracle, nch):
    """a channel passband per lane group (each group's channels share it; the last group ragged): 2, 3, 5 and 16 lane
    groups -- even counts, which a one-filter tuner streams with two lane groups per wave, and odd ones -- one launch"""
    bins = per_group(nch)
    assert sets_per_group(bins) == [1] * sc.lane_groups(nch) and len(set(bins)) > 1
    _stream_vs_blocks(dev, oracle, FS, CRATE, ARATE, bins, N, 5, (1, 5))


@pytest.mark.parametrize("pd2", sorted(sc.MIXED_FILTERS), ids=lambda p: f"PD2={p}")
def test_mixed_filters_in_a_lane_group_stream(dev, oracle, pd2):
    """2, 3 and 4 distinct passbands across the lanes of a lane group -- the same in every group, or a different mix per
    group -- at every audio decimation the stream takes: every k_tuner_stream<PD2, 1, WR_TAPSETS> instance; byte blocks once"""
    fs, crate = DECIMATION_RATES[pd2]
    nch, k, layout, u8 = sc.MIXED_FILTERS[pd2]
    bins = (spread if layout == "spread" else staggered)(nch, k)
    sets = sets_per_group(bins)
    assert max(sets) == k > 1 and (layout == "spread" or len(set(sets)) > 1), sets
    d1 = fs // crate
    k2 = -(-64 // pd2) + 29
    _stream_vs_blocks(dev, oracle, fs, crate, crate // pd2, bins, k2 * pd2 * d1, 5, (1, 5), u8=u8)


@pytest.mark.parametrize("fs,crate,arate", [(240_000, 240_000, 48_000), (480_000, 240_000, 80_000)],
                         ids=["D1=1", "D1=2"])
def test_block_zero_boundary_frames_with_mixed_filters(dev, oracle, fs, crate, arate):
    """D1 = 1 and 2: the first 63 and 32 output frames of block 0 reach into the history before the stream and go to the
    block-boundary role (ddc_body in the post workgroups), with four window copies per wave there too"""
    nch = 130
    bins = spread(nch, 4)
    d1, d2 = fs // crate, crate // arate
    kslow = -(-63 // d1)
    k2 = 50
    assert kslow > 1 and k2 * d2 > kslow
    _stream_vs_blocks(dev, oracle, fs, crate, arate, bins, k2 * d2 * d1, 4, (1, 4))


def test_five_filters_in_a_lane_group_do_not_stream(dev, oracle):
    """five distinct channel filters in one lane group: the per-lane-taps kernel, a launch per block"""
    bins = spread(70, 5)
    assert sets_per_group(bins) == [5, 5]
    _stream_vs_blocks(dev, oracle, FS, CRATE, ARATE, bins, N, 4, (0, 0))


def test_filter_setters_mid_stream(dev, oracle):
    """setPassband on one receiver between blocks: the launch closes at that block boundary and the next block opens
    another; a setter that gives a lane group a FIFTH filter sends the tuner the ordinary way, and one that brings it
    back to four lets it stream again.  The same bits as a launch per block, call for call."""
    nch, nblk = 130, 8
    bins = [1 + c % 4 for c in range(64)] + [1 + c % 2 for c in range(64, nch)]
    moved1, moved2 = 65, 5                        # lane group 1 (2 -> 3 filters) and lane group 0 (4 -> 5 -> 4)
    assert bins[moved2] == 2 and bins[moved1] == 2
    ifs = sc.spread_ifs(FS, nch)
    host_blocks, blocks, submit = sc.device_stream(FS, ifs, N, nblk)
    first = _setter(FS, CRATE, bins)

    def run(stream):
        seen = {}

        def between(t, chans, b):
            got = first(t, chans, b)
            if b in (2, 4, 6):
                seen[b] = t.stream_info()
                if b == 2:
                    t.set_filter(chans[moved1], 0, pb(FS, 3), CRATE)
                elif b == 4:
                    t.set_filter(chans[moved2], 0, pb(FS, 5), CRATE)      # lane group 0: bins 1..5
                else:
                    t.set_filter(chans[moved2], 0, pb(FS, 4), CRATE)      # back to bins 1..4
            return got

        out = sc.play(dev, FS, CRATE, ARATE, ifs, blocks, stream, submit, between=between)
        return out, seen

    one, seen1 = run(False)
    many, seen = run(True)
    assert one["info"][1:] == (0, 0) and all(v[1:] == (0, 0) for v in seen1.values())
    assert seen[2] == (True, 1, 2), seen            # blocks 0, 1: one launch
    assert seen[4] == (True, 2, 4), seen            # blocks 2, 3: the setter closed it, block 2 opened the second
    assert seen[6] == (False, 2, 4), seen           # blocks 4, 5: five filters in lane group 0, a launch per block
    assert many["info"] == (True, 3, 6), many["info"]   # blocks 6, 7: four again, a third launch
    sc.same_bits(one, many)
    final = list(bins)
    final[moved1], final[moved2] = 3, 4
    sc.against_oracle(_yardstick(oracle, FS, CRATE, ARATE, ifs, final), host_blocks, many,
                      sc.passband_probes(final, skip=(moved1, moved2)), sc.covers_passbands(final))


def test_c2_full_size_with_a_passband_per_receiver(dev, oracle):
    """BASELINE config 2 at full size with four channel passbands in every lane group (receiver c: bin 1 + (c // 4) % 4, so
    the carrier receivers, every fourth, take all four): 256 receivers, three resident 4 M-frame blocks through ONE launch;
    the same bits as a launch per block, and three carrier receivers of three passbands against the oracle on the
    stream's first 200 000 frames"""
    import torch
    c2 = synth.C2
    fs, n, crate, arate = c2["input_rate"], c2["block_frames"], c2["chan_rate"], c2["audio_rate"]
    ifs = synth.c2_ifs()
    nblk = 3
    k1 = n // (fs // crate)
    bins = [1 + (c // 4) % 4 for c in range(256)]
    assert sets_per_group(bins) == [4] * 4
    x = synth.fm_stream_torch(n * nblk, fs, ifs[::4], "cuda")
    torch.cuda.synchronize()
    check = (0, 4, 8)                                 # bins 1, 2, 3; carriers of their own

    def run(stream):
        t = Tuner(dev, fs, 256, n, capi.WR_NCO_ROTATE)
        chans = [t.add_receiver(f, c2["chan_passband"], crate, capi.WR_FM, c2["audio_passband"], arate) for f in ifs]
        for c, ch in enumerate(chans):
            t.set_filter(ch, 0, pb(fs, bins[c]), crate)
        t.audio_ring(nblk)
        t.streaming(stream)
        first_iq = {}
        for b in range(nblk):
            t.submit_device(x[2 * n * b: 2 * n * (b + 1)], n)
            if b == 0 and not stream:
                first_iq = {c: t.fetch(chans[c], capi.WR_STAGE_CHAN_IQ, 2 * k1) for c in check}
        info = t.stream_info()
        t.flush()
        got = drain(t, nblk)
        out = dict(got=got, info=info, slots=[t.slot(ch) for ch in chans],
                   iq=[t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1) for ch in chans], state=[t.state(ch) for ch in chans])
        t.destroy()
        return out, first_iq

    one, first_iq = run(False)
    many, _ = run(True)
    assert one["info"][1:] == (0, 0)
    assert many["info"] == (True, 1, nblk), many["info"]
    sc.same_bits(one, many)
    m = 200_000
    xh = x[: 2 * m].cpu().numpy()
    for c in check:
        rx = oracle.Receiver(fs, ifs[c], pb(fs, bins[c]), crate, oracle.FM, c2["audio_passband"], arate)
        wa, wc, _ = rx.run(xh)
        assert wc.size == 2 * (m // (fs // crate)) and wa.size == m // (fs // arate)
        assert np.abs(first_iq[c][: wc.size] - wc).max() <= IQ_ATOL, c
        tol = AUDIO_ATOL * max(1.0, float(np.abs(oracle.lowpass_design(c2["audio_passband"], crate)).sum()))
        assert np.abs(many["got"][0][1][many["slots"][c]][: wa.size] - wa).max() <= tol, c
        assert float(np.abs(wa).max()) > 1e-3
