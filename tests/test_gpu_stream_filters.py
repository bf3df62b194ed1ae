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

from webradio_amd import capi, synth
from webradio_amd.device import Tuner
from test_gpu_stream import (AUDIO_ATOL, DECIMATION_RATES, IQ_ATOL, MODES, _carriers, _drain, _fm_probes,
                             _lane_groups, _passbands, _play, _same_bits, _spread_ifs)

pytestmark = pytest.mark.gpu


def _pb(fs, m):
    """a channel passband in the middle of the reference's frequency bin m (lowpass_maxbin: passband * 32 / rate): bins
    1..5 give five distinct 64-tap filters at every input rate used here"""
    return fs * m // 32 + fs // 64


def _spread(nch, k):
    """k distinct passbands spread across the lanes of every lane group: receiver c takes bin 1 + c % k"""
    return [1 + c % k for c in range(nch)]


def _staggered(nch, k):
    """lane group g mixes k - g % k passbands (k, k - 1, ..., 1), each group a different selection of bins 1..5"""
    out = []
    for c in range(nch):
        g = c // 64
        nk = k - g % k
        out.append(1 + (g + c % nk) % 5)
    return out


def _per_group(nch):
    """one passband per lane group, all channels of a group sharing it, neighbouring groups different"""
    return [1 + (c // 64) % 5 for c in range(nch)]


def _sets_per_group(bins):
    return [len(set(bins[g * 64:(g + 1) * 64])) for g in range(_lane_groups(len(bins)))]


def _setter(fs, crate, bins):
    """_play's `between`: before block 0, every receiver's channel passband (Receiver::channelFilter()->setPassband)"""
    def between(t, chans, b):
        if b == 0:
            for c, ch in enumerate(chans):
                t.set_filter(ch, 0, _pb(fs, bins[c]), crate)
        return []
    return between


def _probes(bins, skip=()):
    """per distinct passband, two receivers of a linear demodulator (AM / USB / LSB: 1-Lipschitz in the channel IQ), in
    different lane groups where there are; plus the FM receivers that carry a carrier (test_gpu_stream._fm_probes)"""
    nch = len(bins)
    out = set(c for c in _fm_probes(nch) if c not in skip)
    for m in sorted(set(bins)):
        mine = [c for c in range(nch) if bins[c] == m and c % 4 != 0 and c not in skip]
        if mine:
            out.add(mine[0])
            other = [c for c in mine if c // 64 != mine[0] // 64]
            out.add(other[-1] if other else mine[-1])
    return sorted(out)


def _against_the_oracle(oracle, fs, crate, arate, ifs, bins, host_blocks, run, probes):
    """the probes' audio of every block and the last block's channel IQ against oracle.Receiver with the probe's OWN
    channel passband, within test_gpu_stream's tolerances; every distinct passband is probed and a carrier is heard"""
    assert run["slots"] == list(range(len(ifs)))           # (receiver c sits in lane group c // 64: the bins above are per slot)
    assert {bins[c] for c in probes} == set(bins)
    _, apb = _passbands(fs, crate, arate)
    loudest = 0.0
    for c in probes:
        rx = oracle.Receiver(fs, ifs[c], _pb(fs, bins[c]), crate, MODES[c % 4], apb, arate)
        if MODES[c % 4] == capi.WR_FM:
            tol = AUDIO_ATOL * max(1.0, float(np.abs(oracle.lowpass_design(apb, crate)).sum()))
        else:
            tol = AUDIO_ATOL
        for b, iq in enumerate(host_blocks):
            wa, wc, _ = rx.run(iq)
            ga = run["got"][b][1][run["slots"][c]]
            assert ga.shape == wa.shape and np.abs(ga - wa).max() <= tol, (c, b, float(np.abs(ga - wa).max()))
            loudest = max(loudest, float(np.abs(wa).max()))
        assert run["iq"][c].shape == wc.shape and np.abs(run["iq"][c] - wc).max() <= IQ_ATOL, c
    assert loudest > 1e-3, loudest


def _stream_vs_blocks(dev, oracle, fs, crate, arate, bins, n, nblk, expect, u8=False):
    """nblk blocks of n frames out of device memory, streamed and with a launch per block: the same bits, the exact
    stream_info() `expect` = (launches, blocks), the probes against the oracle"""
    import torch
    nch = len(bins)
    ifs = _spread_ifs(fs, nch)
    iq = synth.fm_stream(nblk * n, fs, _carriers(ifs), amp=0.1)
    if u8:
        raw = np.clip(np.rint(iq * 128.0 + 128.0), 0, 255).astype(np.uint8)
        iq = oracle.u8_to_float(raw)                       # what the tuner sees (io/rtlsdrtuner.cxx:106)
        x = torch.from_numpy(raw).cuda()
    else:
        x = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    blocks = [(b * n, n) for b in range(nblk)]
    views = [x[2 * off: 2 * (off + m)] for off, m in blocks]

    def submit(t, b, off, m):
        (t.submit_u8_device if u8 else t.submit_device)(views[b], m)

    between = _setter(fs, crate, bins)
    one = _play(dev, fs, crate, arate, ifs, blocks, False, submit, between=between)
    many = _play(dev, fs, crate, arate, ifs, blocks, True, submit, between=between)
    assert one["info"][1:] == (0, 0)
    launches, taken = expect
    assert many["info"] == (launches > 0, launches, taken), many["info"]
    _same_bits(one, many)
    _against_the_oracle(oracle, fs, crate, arate, ifs, bins, [iq[2 * off: 2 * (off + m)] for off, m in blocks], many,
                        _probes(bins))
    return many


FS, CRATE, ARATE = 2_400_000, 240_000, 48_000         # D1 = 10, D2 = 5
N = 100 * 5 * 10                                      # 100 audio frames a block


@pytest.mark.parametrize("nch", [122, 186, 314, 1000], ids=lambda n: f"{_lane_groups(n)}-groups")
def test_a_filter_per_lane_group_streams(dev, oracle, nch):
    """a channel passband per lane group (each group's channels share it; the last group ragged): 2, 3, 5 and 16 lane
    groups -- even counts, which a one-filter tuner streams with two lane groups per wave, and odd ones -- one launch"""
    bins = _per_group(nch)
    assert _sets_per_group(bins) == [1] * _lane_groups(nch) and len(set(bins)) > 1
    _stream_vs_blocks(dev, oracle, FS, CRATE, ARATE, bins, N, 5, (1, 5))


# audio decimation: (receivers, distinct passbands per lane group, how they are laid out, byte blocks)
MIXED = {1: (70, 2, "spread", False), 2: (130, 3, "staggered", False), 3: (200, 4, "spread", False),
         4: (64, 4, "spread", False), 5: (130, 4, "spread", True), 6: (70, 3, "staggered", False),
         8: (130, 2, "spread", False), 10: (200, 4, "staggered", False)}


@pytest.mark.parametrize("pd2", sorted(MIXED), ids=lambda p: f"PD2={p}")
def test_mixed_filters_in_a_lane_group_stream(dev, oracle, pd2):
    """2, 3 and 4 distinct passbands across the lanes of a lane group -- the same in every group, or a different mix per
    group -- at every audio decimation the stream takes: every k_tuner_stream<PD2, 1, WR_TAPSETS> instance; byte blocks once"""
    fs, crate = DECIMATION_RATES[pd2]
    nch, k, layout, u8 = MIXED[pd2]
    bins = (_spread if layout == "spread" else _staggered)(nch, k)
    sets = _sets_per_group(bins)
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
    bins = _spread(nch, 4)
    d1, d2 = fs // crate, crate // arate
    kslow = -(-63 // d1)
    k2 = 50
    assert kslow > 1 and k2 * d2 > kslow
    _stream_vs_blocks(dev, oracle, fs, crate, arate, bins, k2 * d2 * d1, 4, (1, 4))


def test_five_filters_in_a_lane_group_do_not_stream(dev, oracle):
    """five distinct channel filters in one lane group: the per-lane-taps kernel, a launch per block"""
    bins = _spread(70, 5)
    assert _sets_per_group(bins) == [5, 5]
    _stream_vs_blocks(dev, oracle, FS, CRATE, ARATE, bins, N, 4, (0, 0))


def test_filter_setters_mid_stream(dev, oracle):
    """setPassband on one receiver between blocks: the launch closes at that block boundary and the next block opens
    another; a setter that gives a lane group a FIFTH filter sends the tuner the ordinary way, and one that brings it
    back to four lets it stream again.  The same bits as a launch per block, call for call."""
    import torch
    nch, nblk = 130, 8
    bins = [1 + c % 4 for c in range(64)] + [1 + c % 2 for c in range(64, nch)]
    moved1, moved2 = 65, 5                        # lane group 1 (2 -> 3 filters) and lane group 0 (4 -> 5 -> 4)
    assert bins[moved2] == 2 and bins[moved1] == 2
    ifs = _spread_ifs(FS, nch)
    iq = synth.fm_stream(nblk * N, FS, _carriers(ifs), amp=0.1)
    x = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    blocks = [(b * N, N) for b in range(nblk)]
    views = [x[2 * off: 2 * (off + m)] for off, m in blocks]
    first = _setter(FS, CRATE, bins)

    def submit(t, b, off, m):
        t.submit_device(views[b], m)

    def run(stream):
        seen = {}

        def between(t, chans, b):
            got = first(t, chans, b)
            if b in (2, 4, 6):
                seen[b] = t.stream_info()
                if b == 2:
                    t.set_filter(chans[moved1], 0, _pb(FS, 3), CRATE)
                elif b == 4:
                    t.set_filter(chans[moved2], 0, _pb(FS, 5), CRATE)      # lane group 0: bins 1..5
                else:
                    t.set_filter(chans[moved2], 0, _pb(FS, 4), CRATE)      # back to bins 1..4
            return got

        out = _play(dev, FS, CRATE, ARATE, ifs, blocks, stream, submit, between=between)
        return out, seen

    one, seen1 = run(False)
    many, seen = run(True)
    assert one["info"][1:] == (0, 0) and all(v[1:] == (0, 0) for v in seen1.values())
    assert seen[2] == (True, 1, 2), seen            # blocks 0, 1: one launch
    assert seen[4] == (True, 2, 4), seen            # blocks 2, 3: the setter closed it, block 2 opened the second
    assert seen[6] == (False, 2, 4), seen           # blocks 4, 5: five filters in lane group 0, a launch per block
    assert many["info"] == (True, 3, 6), many["info"]   # blocks 6, 7: four again, a third launch
    _same_bits(one, many)
    final = list(bins)
    final[moved1], final[moved2] = 3, 4
    probes = _probes(final, skip=(moved1, moved2))
    _against_the_oracle(oracle, FS, CRATE, ARATE, ifs, final, [iq[2 * off: 2 * (off + m)] for off, m in blocks], many,
                        probes)


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
    assert _sets_per_group(bins) == [4] * 4
    x = synth.fm_stream_torch(n * nblk, fs, ifs[::4], "cuda")
    torch.cuda.synchronize()
    check = (0, 4, 8)                                 # bins 1, 2, 3; carriers of their own

    def run(stream):
        t = Tuner(dev, fs, 256, n, capi.WR_NCO_ROTATE)
        chans = [t.add_receiver(f, c2["chan_passband"], crate, capi.WR_FM, c2["audio_passband"], arate) for f in ifs]
        for c, ch in enumerate(chans):
            t.set_filter(ch, 0, _pb(fs, bins[c]), crate)
        t.audio_ring(nblk)
        t.streaming(stream)
        first_iq = {}
        for b in range(nblk):
            t.submit_device(x[2 * n * b: 2 * n * (b + 1)], n)
            if b == 0 and not stream:
                first_iq = {c: t.fetch(chans[c], capi.WR_STAGE_CHAN_IQ, 2 * k1) for c in check}
        info = t.stream_info()
        t.flush()
        got = _drain(t, nblk)
        out = dict(got=got, info=info, slots=[t.slot(ch) for ch in chans],
                   iq=[t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * k1) for ch in chans], state=[t.state(ch) for ch in chans])
        t.destroy()
        return out, first_iq

    one, first_iq = run(False)
    many, _ = run(True)
    assert one["info"][1:] == (0, 0)
    assert many["info"] == (True, 1, nblk), many["info"]
    _same_bits(one, many)
    m = 200_000
    xh = x[: 2 * m].cpu().numpy()
    for c in check:
        rx = oracle.Receiver(fs, ifs[c], _pb(fs, bins[c]), crate, oracle.FM, c2["audio_passband"], arate)
        wa, wc, _ = rx.run(xh)
        assert wc.size == 2 * (m // (fs // crate)) and wa.size == m // (fs // arate)
        assert np.abs(first_iq[c][: wc.size] - wc).max() <= IQ_ATOL, c
        tol = AUDIO_ATOL * max(1.0, float(np.abs(oracle.lowpass_design(c2["audio_passband"], crate)).sum()))
        assert np.abs(many["got"][0][1][many["slots"][c]][: wa.size] - wa).max() <= tol, c
        assert float(np.abs(wa).max()) > 1e-3
