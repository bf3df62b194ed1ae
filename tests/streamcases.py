"""What the tests of the streaming launch (k_tuner_stream: test_gpu_stream, test_gpu_stream_filters,
test_gpu_stream_long_audio) share: the receivers and carriers of a stream, the probe receivers, ONE play of a list of blocks
through a fresh tuner, and ONE comparison each of a streamed run with a launch per block (same_bits) and with the oracle
(against_oracle).  The tolerances are tests/tunercases.py's.

Receiver c of every tuner here demodulates MODES[c % 4] -- FM is c % 4 == 0, which the probe arithmetic relies on (the
tuner tests' own MODES are in another order).

This is not a test module: pytest does not rewrite its asserts, so every assert says what it compared."""
import numpy as np

import launch_plan
from tunercases import AUDIO_ATOL, IQ_ATOL, LINEAR_ATOL, OracleChain, bits, bits_f32, drain
from webradio_amd import capi, synth
from webradio_amd.device import Tuner

MODES = (capi.WR_FM, capi.WR_USB, capi.WR_AM, capi.WR_LSB)     # receiver c demodulates MODES[c % 4]

# (fs, chan_rate) per audio decimation: D1 = 10, 12, 20, 8, 16, 8, 16, 5
DECIMATION_RATES = {1: (2_400_000, 240_000), 2: (2_400_000, 200_000), 3: (2_400_000, 120_000), 4: (2_048_000, 256_000),
                    5: (2_400_000, 150_000), 6: (1_920_000, 240_000), 8: (2_048_000, 128_000), 10: (2_400_000, 480_000)}
LANE_CASES = {"odd": 130, "even": 70}         # 3 and 2 lane groups of 64, the last one ragged

# The case tables whose receiver counts and layouts the probe selectors below must cover (tests/test_streamcases.py holds them
# to that without a GPU).
# test_gpu_stream.test_stream_block_edges -- id: (fs, chan_rate, audio_rate, receivers, audio frames per block or None for the
# smallest block a launch takes, (min_run, run, drain_run, how) wrk_tuner_stream picks for n_post = 252 (MI355X: 256 CUs) or None)
BLOCK_EDGE_CASES = {
    "smallest-D1=1": (240_000, 240_000, 48_000, 70, None, None),            # 65 frames, k2 = 13: under one tile
    "smallest-D1=2": (480_000, 240_000, 80_000, 130, None, None),           # 132 frames, k2 = 22: a ragged second tile
    "smallest-D1=3": (720_000, 240_000, 60_000, 70, None, None),            # 192 frames, k2 = 16: exactly one tile
    "under-one-tile": (2_400_000, 240_000, 30_000, 130, 9, None),
    "run-1-ragged": (2_400_000, 240_000, 48_000, 40, 60, (1, 1, 1, "min")),
    "run-2": (2_400_000, 240_000, 80_000, 100, 790, (1, 2, 1, "min+loop")),
    "run-3": (2_048_000, 256_000, 64_000, 300, 393, (1, 3, 1, "min+loop+loop")),
    "run-4": (2_400_000, 60_000, 60_000, 40, 4790, (2, 4, 2, "long+loop")),
    "long-runs": (2_400_000, 60_000, 30_000, 100, 3595, (2, 4, 2, "long")),
    "16-groups": (2_400_000, 240_000, 48_000, 1000, 100, None),
    "17-groups": (2_400_000, 240_000, 48_000, 1025, 100, None),
}
# test_gpu_stream_filters.test_a_filter_per_lane_group_streams: receivers (2, 3, 5 and 16 lane groups, the last ragged)
FILTER_PER_GROUP_COUNTS = [122, 186, 314, 1000]
# test_gpu_stream_filters.test_mixed_filters_in_a_lane_group_stream -- audio decimation: (receivers, distinct passbands per lane
# group, how they are laid out, byte blocks)
MIXED_FILTERS = {1: (70, 2, "spread", False), 2: (130, 3, "staggered", False), 3: (200, 4, "spread", False),
                 4: (64, 4, "spread", False), 5: (130, 4, "spread", True), 6: (70, 3, "staggered", False),
                 8: (130, 2, "spread", False), 10: (200, 4, "staggered", False)}
# test_gpu_stream_long_audio.test_long_audio_filter_with_channel_passbands_per_receiver -- audio taps: (audio decimation,
# receivers, distinct channel passbands per lane group, how they are laid out)
LONG_MIXED_FILTERS = {128: [(5, 130, 4, "spread"), (10, 70, 3, "staggered"), (1, 200, 2, "spread")],
                      256: [(3, 130, 4, "staggered"), (1, 70, 2, "spread"), (2, 200, 3, "spread")]}


# ---- launch geometry --------------------------------------------------------------------------------------------------------------

def lane_groups(nch):
    return (nch + 63) // 64


def ng(groups):
    """wrk_tuner_stream: k_tuner_stream<PD2, 1> for an odd lane-group count, <PD2, 2> for an even one"""
    return 1 if groups & 1 else 2


def post_tiling(k2, groups, n_post):
    """wrk_tuner_stream's cut of one block's post stage, from the rule itself (wr_plan.h: wrp_post_tiling_stream, which says
    which of its branches it took): (min_run, run, drain_run, how run was chosen)"""
    t = launch_plan.stream_tiling(k2, groups, n_post)
    return t.min_run, t.run, t.drain_run, ("long" if t.long_runs else "min") + "+loop" * t.widened


def n_post():
    """post workgroups of a streaming launch on this device (wr_plan.h: wrp_stream_roles: one slot per CU, less four, whether
    the launch has two or three workgroups per CU -- two, the fewest a launch exists with, is what is asked here)"""
    import torch
    return launch_plan.stream_roles(2, torch.cuda.get_device_properties(0).multi_processor_count)[1]


# ---- receivers, passbands, carriers -------------------------------------------------------------------------------------------------

def passbands(fs, crate, arate):
    """(channel, audio) passband.  The reference's 64-tap LowPass keeps the frequency bins below passband * 32 / rate
    (lowpass_maxbin): a channel passband of fs / 16 keeps two at every input rate, arate / 3 at least one up to D2 = 10."""
    return fs // 16, arate // 3


def spread_ifs(fs, nch):
    step = int(0.9 * fs / nch)
    return [(c - nch // 2) * step + 37 for c in range(nch)]


def fm_probes(nch):
    """the FM receivers that carry a carrier: the first, and the last FM one, in the ragged last lane group"""
    return [0, (nch - 1) // 4 * 4]


def carriers(ifs):
    return [ifs[c] for c in fm_probes(len(ifs))]


def pb(fs, m):
    """a channel passband in the middle of the reference's frequency bin m (lowpass_maxbin: passband * 32 / rate): bins
    1..5 give five distinct 64-tap filters at every input rate used here"""
    return fs * m // 32 + fs // 64


def spread(nch, k):
    """k distinct passbands spread across the lanes of every lane group: receiver c takes bin 1 + c % k"""
    return [1 + c % k for c in range(nch)]


def staggered(nch, k):
    """lane group g mixes k - g % k passbands (k, k - 1, ..., 1), each group a different selection of bins 1..5"""
    out = []
    for c in range(nch):
        g = c // 64
        nk = k - g % k
        out.append(1 + (g + c % nk) % 5)
    return out


def per_group(nch):
    """one passband per lane group, all channels of a group sharing it, neighbouring groups different"""
    return [1 + (c // 64) % 5 for c in range(nch)]


def sets_per_group(bins):
    return [len(set(bins[g * 64:(g + 1) * 64])) for g in range(lane_groups(len(bins)))]


# ---- probe receivers, and what a probe set must cover -------------------------------------------------------------------------------

def probes(nch):
    """receivers 0-3 (every mode), an AM / USB / LSB one in every lane group, the FM probes and the last receiver.  (Only the FM
    probes have a carrier of their own, far from each other: FM's arctangent is well conditioned only where one carrier
    dominates the channel; the other demodulators are linear or 1-Lipschitz in the channel IQ.)"""
    one_per_group = {64 * g + 1 + (g % 3) for g in range(lane_groups(nch))}
    return sorted({0, 1, 2, 3, nch - 1} | {c for c in one_per_group if c < nch} | set(fm_probes(nch)))


def group_probes(nch):
    """all four demodulators in every lane group (the ragged last one too), and probes(nch): the FM ones carry the carriers"""
    out = set(probes(nch))
    for g in range(lane_groups(nch)):
        top = min(64 * g + 63, nch - 1)
        for m in range(4):
            mine = [c for c in range(64 * g, top + 1) if c % 4 == m]
            if mine:
                out.add(mine[len(mine) // 2])
    return sorted(out)


def passband_probes(bins, skip=()):
    """per distinct passband, two receivers of a linear demodulator (AM / USB / LSB: 1-Lipschitz in the channel IQ), in
    different lane groups where there are; plus the FM receivers that carry a carrier (fm_probes)"""
    nch = len(bins)
    out = set(c for c in fm_probes(nch) if c not in skip)
    for m in sorted(set(bins)):
        mine = [c for c in range(nch) if bins[c] == m and c % 4 != 0 and c not in skip]
        if mine:
            out.add(mine[0])
            other = [c for c in mine if c // 64 != mine[0] // 64]
            out.add(other[-1] if other else mine[-1])
    return sorted(out)


def covers_groups_and_modes(nch):
    """every lane group (the ragged last too) and every demodulator"""
    def check(run, chosen):
        groups = {run["slots"][c] // 64 for c in chosen}
        assert groups == set(range(lane_groups(nch))), "probes %s sit in lane groups %s of %d" % (chosen, sorted(groups), lane_groups(nch))
        modes = {c % 4 for c in chosen}
        assert modes == {0, 1, 2, 3}, "probes %s have the demodulators %s only" % (chosen, sorted(modes))
    return check


def covers_passbands(bins):
    """every distinct channel passband (receiver c sits in lane group c // 64: `bins` is per slot)"""
    def check(run, chosen):
        assert run["slots"] == list(range(len(bins))), "receiver c does not sit in slot c: %s" % (run["slots"],)
        seen = {bins[c] for c in chosen}
        assert seen == set(bins), "probes %s have the passbands %s of %s" % (chosen, sorted(seen), sorted(set(bins)))
    return check


def covers_modes_in_groups(nch):
    """every demodulator in every lane group (receiver c sits in slot c; a ragged last lane group may be too short to hold
    all four)"""
    def check(run, chosen):
        assert run["slots"] == list(range(nch)), "receiver c does not sit in slot c: %s" % (run["slots"],)
        seen, every = {(c // 64, c % 4) for c in chosen}, {(c // 64, c % 4) for c in range(nch)}
        assert seen == every, "probes %s leave out (lane group, demodulator) %s" % (chosen, sorted(every - seen))
    return check


# ---- the play ---------------------------------------------------------------------------------------------------------------------

def play(dev, fs, crate, arate, ifs, blocks, stream, submit, between=None, ring=None, take_every=None, before=None,
         fir_lengths=None, cpbs=None, apbs=None):
    """Submit `blocks` ((offset, frames) into the stream) to a fresh tuner, streaming or with one launch per block, taking every
    block's audio out of the ring.  stream: what Tuner.streaming() is given, or a callable(t, b) that sets it itself before
    block b is submitted.  between(t, chans, b): called before block b is submitted, returns the ring entries it took;
    before(): called once, right before the first submit.  fir_lengths: every receiver's (channel, audio) filter lengths;
    cpbs / apbs: a channel / an audio passband per receiver in place of passbands().  Returns a dict: the ring entries
    (seq, audio), the slots, the last block's channel IQ and every receiver's state after a flush, stream_info before it, the
    host-block count and the long-run count after it."""
    nch = len(ifs)
    t = Tuner(dev, fs, nch, max(n for _, n in blocks), capi.WR_NCO_ROTATE)
    cpb, apb = passbands(fs, crate, arate)
    chans = [t.add_receiver(f, cpbs[c] if cpbs else cpb, crate, MODES[c % 4], apbs[c] if apbs else apb, arate,
                            fir_lengths=fir_lengths)
             for c, f in enumerate(ifs)]
    t.audio_ring(ring or len(blocks))
    if not callable(stream):
        t.streaming(stream)
    got = []
    if before is not None:
        before()
    for b, (off, n) in enumerate(blocks):
        if between is not None:
            got += between(t, chans, b)
        if callable(stream):
            stream(t, b)
        submit(t, b, off, n)
        if take_every and t.ring_stats()[0] >= take_every:
            got += drain(t, t.ring_stats()[0])
    info = t.stream_info()
    t.flush()
    got += drain(t, len(blocks) - len(got))
    k1 = blocks[-1][1] * crate // fs
    out = dict(got=got, info=info, host=t.stream_host_blocks(), slots=[t.slot(c) for c in chans],
               iq=[t.fetch(c, capi.WR_STAGE_CHAN_IQ, 2 * k1) for c in chans],
               state=[t.state(c) for c in chans])
    out["long"] = t.stream_long_blocks()           # (counted when the closed launch is checked: the state reads waited for it)
    t.destroy()
    return out


# ---- the comparisons --------------------------------------------------------------------------------------------------------------

def same_bits(one, many):
    """the streamed run against the launch-per-block run: every block's audio on EVERY receiver, the last block's channel IQ
    and every receiver's state"""
    seqs = [[s for s, _ in r["got"]] for r in (one, many)]
    assert seqs[0] == seqs[1] == list(range(len(one["got"]))), "ring sequence numbers %s and %s" % tuple(seqs)
    assert one["slots"] == many["slots"], "slots %s and %s" % (one["slots"], many["slots"])
    rows = one["slots"]
    for b, ((_, u), (_, v)) in enumerate(zip(one["got"], many["got"])):
        assert u.shape == v.shape, "block %d: audio of shape %s and %s" % (b, u.shape, v.shape)
        bad = np.argwhere(bits(u[rows]) != bits(v[rows]))
        assert bad.size == 0, "block %d: %d audio samples differ, the first at (receiver, frame) %s" % (b, len(bad), bad[0])
    for c, (u, v) in enumerate(zip(one["iq"], many["iq"])):
        assert u.size and u.shape == v.shape, "receiver %d: channel IQ of shape %s and %s" % (c, u.shape, v.shape)
        bad = np.flatnonzero(bits(u) != bits(v))
        assert bad.size == 0, "receiver %d: %d channel-IQ floats of the last block differ, the first at %d" % (c, bad.size, bad[0])
    for c, ((p1, v1), (p2, v2)) in enumerate(zip(one["state"], many["state"])):
        assert p1 == p2, "receiver %d: NCO phase %d and %d" % (c, p1, p2)
        assert np.array_equal(bits_f32(v1), bits_f32(v2)), "receiver %d: the detector's previous frame %s and %s" % (c, v1, v2)


class ProbeOracle:
    """The probes' yardstick.  l2 None: oracle.Receiver (64-tap filters), AM / USB / LSB audio within AUDIO_ATOL.  l2 taps of
    audio filter: the oracle's mixer -> LowPass(64, D1) -> demodulator -> LowPass(l2, D2) chain (tunercases.OracleChain), AM /
    USB / LSB audio within LINEAR_ATOL x sum|h2|.  cpbs / apbs: the probe's OWN channel / audio passband in place of passbands()."""

    def __init__(self, oracle, fs, crate, arate, ifs, l2=None, cpbs=None, apbs=None):
        self.oracle, self.fs, self.crate, self.arate, self.ifs, self.l2 = oracle, fs, crate, arate, ifs, l2
        cpb, apb = passbands(fs, crate, arate)
        self.cpbs, self.apbs = cpbs or [cpb] * len(ifs), apbs or [apb] * len(ifs)

    def rx(self, c):
        o, fs, crate, cpb, pb2 = self.oracle, self.fs, self.crate, self.cpbs[c], self.apbs[c]
        bins = o.lowpass_maxbin(cpb, fs), o.lowpass_maxbin_n(self.l2, pb2, crate) if self.l2 else o.lowpass_maxbin(pb2, crate)
        assert min(bins) >= 1, "receiver %d: a filter that passes nothing (bins %s)" % (c, bins)
        if self.l2 is None:
            return o.Receiver(fs, self.ifs[c], cpb, crate, MODES[c % 4], pb2, self.arate)
        omode = {capi.WR_FM: o.FM, capi.WR_USB: o.USB, capi.WR_AM: o.AM, capi.WR_LSB: o.LSB}
        return OracleChain(o, fs, self.ifs[c], 64, cpb, fs // crate, omode[MODES[c % 4]], self.l2, pb2, crate // self.arate)

    def audio_taps(self, c):
        return self.oracle.lowpass_design(self.apbs[c], self.crate, self.l2 or 64)

    def tol_linear(self, gain2):
        return AUDIO_ATOL if self.l2 is None else LINEAR_ATOL * gain2


def against_oracle(yardstick, host_blocks, run, chosen, covers=None, check_blocks=None):
    """The probe receivers `chosen`: their audio of every block (or of `check_blocks`) and the last block's channel IQ against
    the oracle on the same input.  yardstick: a ProbeOracle -- rx(c) is the probe's chain (run(iq) -> audio,
    channel IQ, ...), audio_taps(c) its audio filter h2, tol_linear(max(1, sum|h2|)) the bound on AM / USB / LSB audio; FM
    audio is held to AUDIO_ATOL x max(1, sum|h2|): the audio filter's gain over the demodulator's differences.  covers(run,
    chosen) asserts what the probe set must cover, first.  At least one probe carries a carrier."""
    if covers is not None:
        covers(run, chosen)
    loudest = 0.0
    for c in chosen:
        rx = yardstick.rx(c)
        gain2 = max(1.0, float(np.abs(yardstick.audio_taps(c)).sum()))
        tol = AUDIO_ATOL * gain2 if MODES[c % 4] == capi.WR_FM else yardstick.tol_linear(gain2)
        wc = None
        for b, iq in enumerate(host_blocks):
            wa, wc, _ = rx.run(iq)
            if check_blocks is None or b in check_blocks:
                ga = run["got"][b][1][run["slots"][c]]
                assert ga.shape == wa.shape, "receiver %d, block %d: audio of shape %s, the oracle's %s" % (c, b, ga.shape, wa.shape)
                err = float(np.abs(ga - wa).max())
                assert err <= tol, "receiver %d (mode %d), block %d: audio off by %.4g, bound %.4g" % (c, MODES[c % 4], b, err, tol)
                loudest = max(loudest, float(np.abs(wa).max()))
        gc = run["iq"][c]
        assert gc.shape == wc.shape, "receiver %d: last block's channel IQ of shape %s, the oracle's %s" % (c, gc.shape, wc.shape)
        err = float(np.abs(gc - wc).max())
        assert err <= IQ_ATOL, "receiver %d: last block's channel IQ off by %.4g, bound %.4g" % (c, err, IQ_ATOL)
    assert loudest > 1e-3, "no carrier was heard: the probes' %s loudest audio sample is %.4g (want > 1e-3)" % (chosen, loudest)


def device_stream(fs, ifs, n, nblk, amp=0.1, u8_from=None):
    """nblk blocks of n frames of the carriers' stream (carriers(ifs)) resident in device memory -- u8_from: as bytes
    (io/rtlsdrtuner.cxx:106's format; the oracle module given converts them back): (the blocks on the host as the tuner sees
    them, play()'s `blocks`, play()'s `submit`)"""
    import torch
    iq = raw = synth.fm_stream(nblk * n, fs, carriers(ifs), amp=amp)
    if u8_from is not None:
        raw = np.clip(np.rint(iq * 128.0 + 128.0), 0, 255).astype(np.uint8)
        iq = u8_from.u8_to_float(raw)
    x = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    blocks = [(b * n, n) for b in range(nblk)]
    views = [x[2 * off: 2 * (off + m)] for off, m in blocks]            # (sliced ahead: the submits go back to back)

    def submit(t, b, off, m):
        (t.submit_device if u8_from is None else t.submit_u8_device)(views[b], m)
    return [iq[2 * off: 2 * (off + m)] for off, m in blocks], blocks, submit


def stream_vs_blocks(dev, yardstick, fs, crate, arate, ifs, n, nblk, expect, chosen, covers, u8=False, between=None,
                     fir_lengths=None):
    """nblk blocks of n frames out of device memory (u8: as bytes), streamed and with a launch per block on fresh tuners: the
    exact stream_info() tuple (`expect`: one tuple, or a set of admissible ones -- a silent fall-back to a launch per block
    fails), the same bits, the probes `chosen` against the oracle (against_oracle).  between: play()'s, for setters.  Returns
    the streamed run."""
    host_blocks, blocks, submit = device_stream(fs, ifs, n, nblk, u8_from=yardstick.oracle if u8 else None)
    one = play(dev, fs, crate, arate, ifs, blocks, False, submit, between=between, fir_lengths=fir_lengths)
    many = play(dev, fs, crate, arate, ifs, blocks, True, submit, between=between, fir_lengths=fir_lengths)
    assert one["info"] == (False, 0, 0), "stream_info() %s of a tuner that was not asked to stream" % (one["info"],)
    print("stream_info", fir_lengths, crate // arate, len(ifs), n, many["info"])
    admissible = {expect} if isinstance(expect, tuple) else expect
    assert many["info"] in admissible, "stream_info() %s, expected %s" % (many["info"], sorted(admissible))
    same_bits(one, many)
    against_oracle(yardstick, host_blocks, many, chosen, covers)
    return many
