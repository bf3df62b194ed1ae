"""Without a GPU: the scripts of tests/tuner_model.py hold what test_gpu_scripts.py relies on, and the model is consistent
with itself -- so that a script that passes on the GPU has said something, and a model that disagrees with the GPU is not
simply a model that disagrees with its own parts."""
import hashlib

import numpy as np

import tuner_model as tm
from tuner_model import AM, FM, LSB, USB
from tunercases import bits_f32


# ---- the scripts ----------------------------------------------------------------------------------------------------------------

def test_every_operation_kind_occurs():
    seeds = list(tm.fuzz_seeds())
    total = {k: 0 for k in tm.ALL_KINDS}
    first, short = {k: 0 for k in tm.PUSH_KINDS}, {k: 0 for k in tm.BANK_HISTORY}
    for seed in seeds:
        script = tm.make_script(seed)
        assert script == tm.make_script(seed)                            # a pure function of the seed
        st = tm.script_stats(script)
        for k, n in st["kinds"].items():
            total[k] += n
        assert st["run"] >= 3, seed                                       # three streamable blocks in a row
        assert st["agc_on"] >= 1 and st["agc_off"] >= 1, seed             # a stretch with AGC on and one with it off
        assert st["reseated"] >= 1, seed                                  # a remove, then an add into the slot it left
        assert min(st["latched"]) >= 1, (seed, st["latched"])             # every bank latches a window
        # the receiver seated in the slot has its AGC on in a submit, after the one that left had run with its AGC on -- in
        # every seed; the same with a squelch in every other seed
        assert st["reseated_agc"] >= 1, seed
        assert st["reseated_squelch"] >= 1 or seed % 2, seed
        assert st["asked"] >= 1, seed                                     # a setting changed, then asked before the next submit
        assert len([op for op in script["ops"] if op[0] not in tm.BANK_KINDS]) <= 100, (seed, len(script["ops"]))
        assert len(script["ops"]) <= OPS_WITH_BANKS, (seed, len(script["ops"]))
        assert sum(n for _, n in script["cuts"]) == script["total"]
        assert max(n for _, n in script["cuts"]) <= script["max_block"]
        # the row banks: every push kind in every seed; a voice_ctl between a submit and its push; a row muted, pushed, and
        # pushed un-muted again
        assert not [k for k in tm.PUSH_KINDS if st["kinds"][k] < 1], (seed, st["kinds"])
        assert st["ctl_pushed"] >= 1 and st["ctl_late"] >= 1 and st["unmuted"] >= 1, (seed, st)
        for k, n in st["first"].items():
            first[k] += n
        for k, n in st["short"].items():
            short[k] += n
    print("first after a submit: %s; pushes shorter than the history: %s" % (first, short))
    if len(seeds) >= 8:                                                   # (the kinds take turns over the seeds)
        assert not [k for k, n in total.items() if n < 2], total
        assert min(first.values()) >= 1, first                            # each push kind is the first getter after a submit
        assert short["resamp"] >= 1 and short["voice"] >= 1, short        # ... and takes each history writer's short branch


OPS_WITH_BANKS = 150          # at most 100 operations of the first pass, and the three banks at up to 14 pushed submits of them


def test_the_banks_leave_the_scripts_as_they_were():
    """the second pass only adds: without its kinds a script's operations are the first pass's, which draws nothing from the
    second pass's generator -- and everything but the operations is the first pass's too"""
    for seed in tm.fuzz_seeds():
        with_banks, without = tm.make_script(seed), tm.make_script(seed, banks=False)
        assert [op for op in with_banks["ops"] if op[0] not in tm.BANK_KINDS] == without["ops"], seed
        assert not [op for op in without["ops"] if op[0] in tm.BANK_KINDS], seed
        assert {k: v for k, v in with_banks.items() if k != "ops"} == {k: v for k, v in without.items() if k != "ops"}, seed
        if seed in FIRST_PASS:                                            # ... as it was before there was a second pass
            assert hashlib.sha256(repr(without["ops"]).encode()).hexdigest()[:16] == FIRST_PASS[seed], seed


# sha256(repr(ops))[:16] of make_script(seed)["ops"] as the commit before the second pass made them
FIRST_PASS = {0: "b097297aaf3d4cf0", 1: "6c5638663cc57431", 2: "807f223e6065ba2a", 3: "0f2ec1c02aadbc66",
              4: "28842b759bca081a", 5: "14016c716da1ad20", 6: "b8977a6c6ad7d31f", 7: "db209ea61d101c23"}


def last_submit(ops, i):
    return max(j for j in range(i) if ops[j][0] == "submit")


def next_submit(ops, i):
    return min([j for j in range(i, len(ops)) if ops[j][0] == "submit"] or [len(ops)])


def test_what_a_script_guarantees():
    for seed in tm.fuzz_seeds():
        script = tm.make_script(seed)
        ops = script["ops"]
        assert len(script["sq_set"]) <= 8 and len(script["agc_set"]) <= 8
        assert not [c for c in script["sq_set"] + script["agc_set"] if c % 4 == 1]
        assert script["carriers"] == [script["ifs"][c] for c in script["sq_set"]]
        live, pushed, submitted = set(range(script["nrx"])), set(), False
        for i, op in enumerate(ops):
            if op[0] == "set_mode" and op[2] == FM or op[0] == "add" and op[4] == FM:
                assert op[1] % 4 == 1, (seed, op)                         # only receivers 1 mod 4 are ever FM
            if op[0] == "set_if":
                assert op[1] not in script["sq_set"], (seed, op)          # a squelched receiver stays on its carrier
            if op[0] in ("squelch_on", "squelch_thr", "squelch_off"):
                assert op[1] in script["sq_set"]
            if op[0] in ("agc_on", "agc_new", "agc_off"):
                assert op[1] in script["agc_set"]
            if op[0] == "add":
                assert ops[i + 1] == ("bank_reset", op[2]), (seed, i)
                live.add(op[1])
            if op[0] == "reset_history":
                assert ops[i + 1][0] == "bank_reset" and ops[i + 1][1] >= 0, (seed, i)
            if op[0] == "seek":
                assert ops[i + 1] == ("bank_reset", -1), (seed, i)
            if op[0] == "remove":
                live.remove(op[1])
                continue
            if op[0] == "submit":
                pushed, submitted = set(), True
            elif len(op) > 1 and op[0] not in ("bank_reset", "seek", "spectra", "tones", "tones_again", "voice_ctl"):
                assert op[1] in live, (seed, i, op)                       # no operation names a receiver that is gone
            if op[0] in tm.PUSH_KINDS:
                assert submitted and op[0] not in pushed, (seed, i)       # at most one push per bank and submit ...
                assert {"tones"} & {o[0] for o in ops[last_submit(ops, i): next_submit(ops, i)]}, (seed, i)   # ... where the tones are pushed
                pushed.add(op[0])
            if op[0] in tm.BANK_KINDS and op[0].endswith("_again"):
                assert op[0][:-6] in pushed, (seed, i)
            if op[0] == "voice_ctl":
                assert 0 <= op[1] < tm.slot_rows(script["max_channels"]) and (op[2] & 0xFF) < tm.VOICE_FILTERS and not op[2] >> 9
                assert i == 0 or ops[i - 1][0] != "submit" or ops[i + 1][0] != "submit", (seed, i)   # never inside a run of blocks
            if op[0] == "tones":
                assert submitted and op[1] not in pushed, (seed, i)       # at most one push per bank and submit
                pushed.add(op[1])
            if op[0] == "tones_again":
                assert op[1] in pushed, (seed, i)
        assert len(live) == script["nrx"]


def test_the_banks_say_something_on_the_model():
    """the scripts played on the model alone: what the GPU plays compare with is not all zeros and not all alike"""
    zero_out = 0
    for seed in tm.fuzz_seeds():
        script = tm.make_script(seed)
        play = tm.ModelPlay(script, tm.signal(script["total"], script["carriers"], seed))
        evals, agrees, frames, chained, muted_rows = 0, set(), 0, 0, 0
        for op in script["ops"]:
            if op[0] in tm.GETTER_KINDS:                                  # (they change nothing, and tones_np walks rows in Python)
                continue
            got = play.do(op)
            plain =[r.slot for c, r in play.m.rxs.items() if c % 4 != 1]          # receivers that are never FM
            if op[0] == "resamp":
                frames += got[0]
                assert all(got[1][s].shape == (got[0],) for s in got[1])
            elif op[0] == "dcs":
                evals = max([evals] + [got[s][3] for s in plain])
                agrees |= {int(a) for s in plain for a in got[s][0].reshape(-1)}
            elif op[0] == "voice":
                chained += got[1]
                muted_rows += sum(1 for s in plain if play.rb.voice.ctl[s] & tm.voice_np.MUTE and not got[0][s].any())
                k2 = play.m.audio_rows(play.rows).shape[1]
                assert all(got[0][s].shape == (k2,) and got[2][s].shape == (got[1],) for s in got[0])
        # a never-FM row of the DCS bank was evaluated, and the bank does not say the same of every row and code
        assert evals >= 1 and len(agrees) >= 2, (seed, evals, agrees)
        assert frames > 0 and chained > 0 and muted_rows >= 1, (seed, frames, chained, muted_rows)
        zero_out += play.rb.zero_out                                      # (allowed: a push may yield no frame)
    print("pushes that yielded no frame: %d" % zero_out)


# ---- the model ------------------------------------------------------------------------------------------------------------------

D2, Q = 5, tm.D1 * 5
IFS = [-50_321, -25_000 + 321, 321, 25_321, 50_321]
MODES = [AM, FM, USB, LSB, AM]


def _model(agc=True):
    m = tm.TunerModel(tm.FS, 32768.0)
    for c, (f, mode) in enumerate(zip(IFS, MODES)):
        m.add(c, c, f, 128_000, tm.CHAN_RATE, mode, tm.AUDIO_PASSBAND, tm.CHAN_RATE // D2)
    m.set_squelch(0, -46.0)
    m.set_af_gain(3, 6.0)
    if agc:
        m.set_agc(2, (-12.0, 20.0, 60.0))
        m.set_agc(0, (-6.0, 5.0, 40.0))
    return m


def _changes(m, at, agc=True):
    """setters at the boundaries every cut below shares: audio frames 16 and 32"""
    if at == 16:
        m.set_if(4, 77_777)
        m.set_mode(2, LSB)
        m.set_chan_passband(3, 96_000)
        m.set_squelch(0, -44.0)
        if agc:
            m.set_agc(2, (-20.0, 60.0, 30.0))
    if at == 32:
        m.set_af_gain(3, -3.5)
        m.set_mode(4, USB)
        if agc:
            m.set_agc(0, None)


def _play_cuts(cuts, iq, agc=True):
    m = _model(agc)
    out, at = {c: [] for c in range(5)}, 0
    for frames in cuts:
        _changes(m, at, agc)
        m.submit(iq[2 * at * Q: 2 * (at + frames) * Q])
        at += frames
        for c in out:
            assert m.audio(c).size == frames
            out[c].append(m.audio(c))
    return {c: np.concatenate(a) for c, a in out.items()}, m


def test_cut_invariance_of_the_model():
    """the same stream, the same setters at the same frames, cut into whole blocks in three ways -- blocks of one audio frame
    and blocks shorter than the audio filter's history among them: the same audio bits on the receivers that are not FM"""
    iq = tm.signal(48 * Q, [IFS[0], IFS[2]], seed=1)
    whole, m0 = _play_cuts([16, 16, 16], iq)
    assert np.any(whole[0] == 0.0) and np.any(whole[0] != 0.0)            # the squelch closes and opens
    for cuts in ([5, 11, 7, 9, 16], [16, 3, 13, 2, 1, 13], [1, 15, 16, 10, 6]):
        parts, m = _play_cuts(cuts, iq)
        for c in (0, 2, 3, 4):
            assert np.array_equal(bits_f32(parts[c]), bits_f32(whole[c])), (cuts, c)
        assert np.abs(parts[1] - whole[1]).max() <= m.fm_tolerance(1)
        for c in range(5):
            assert m.phase(c) == m0.phase(c) and m.get_agc(c) == m0.get_agc(c)


def test_reset_equals_fresh():
    iq = tm.signal(40 * Q, [IFS[0]], seed=2)
    m = _model()
    m.submit(iq[: 2 * 20 * Q])
    for c in range(5):
        m.reset_history(c)
    phases = [m.phase(c) for c in range(5)]
    prevs = [(m.rxs[c].rx.s.prev_i, m.rxs[c].rx.s.prev_q) for c in range(5)]
    assert any(p != (0.0, 0.0) for p in prevs) and any(phases)
    m.submit(iq[2 * 20 * Q:])
    for c in range(5):
        rx = tm.oracle.Receiver(tm.FS, IFS[c], 128_000, tm.CHAN_RATE, MODES[c], tm.AUDIO_PASSBAND, tm.CHAN_RATE // D2)
        rx.s.phase = phases[c]
        rx.s.prev_i, rx.s.prev_q = prevs[c]
        wa, wc, _ = rx.run(iq[2 * 20 * Q:])
        assert np.array_equal(bits_f32(m.chan_iq(c)), bits_f32(wc)), c
        if c in (1, 4):                                                   # no squelch, af_gain or AGC: the scale alone
            assert np.array_equal(bits_f32(m.audio(c)), bits_f32(wa * np.float32(32768.0))), c
    # ... and the whole receiver, squelch, AGC (from floor again) and af_gain included, is a fresh model's given the same two
    m2 = _model()
    for c in range(5):
        m2.rxs[c].rx.s.phase = phases[c]
        m2.rxs[c].rx.s.prev_i, m2.rxs[c].rx.s.prev_q = prevs[c]
    m2.submit(iq[2 * 20 * Q:])
    for c in range(5):
        assert np.array_equal(bits_f32(m.audio(c)), bits_f32(m2.audio(c))), c
        assert m.get_agc(c) == m2.get_agc(c)
    assert m.get_agc(2)[0] is True and m.get_agc(0)[0] is True


def test_agc_off_changes_nothing():
    iq = tm.signal(48 * Q, [IFS[0], IFS[2]], seed=3)
    with_agc, m = _play_cuts([16, 16, 16], iq, agc=True)
    without, _ = _play_cuts([16, 16, 16], iq, agc=False)
    for c in (1, 3, 4):                                                   # never had an AGC
        assert np.array_equal(bits_f32(with_agc[c]), bits_f32(without[c])), c
    assert not np.array_equal(bits_f32(with_agc[2]), bits_f32(without[2]))      # the AGC did something
    assert not np.array_equal(bits_f32(with_agc[0][:32]), bits_f32(without[0][:32]))
    assert np.array_equal(bits_f32(with_agc[0][32:]), bits_f32(without[0][32:]))   # off from frame 32: the plain receiver's bits
    assert m.get_agc(0)[0] is False and m.get_agc(2)[0] is True


def test_the_model_mends_what_a_change_of_block_size_breaks():
    """quirk Q7 stays out of the model: a bare oracle.Receiver fed the same cuts does lose its history"""
    iq = tm.signal(32 * Q, [IFS[0]], seed=4)
    rx = tm.oracle.Receiver(tm.FS, IFS[2], 128_000, tm.CHAN_RATE, USB, tm.AUDIO_PASSBAND, tm.CHAN_RATE // D2)
    whole = rx.run(iq)[0]
    rx = tm.oracle.Receiver(tm.FS, IFS[2], 128_000, tm.CHAN_RATE, USB, tm.AUDIO_PASSBAND, tm.CHAN_RATE // D2)
    bare = np.concatenate([rx.run(iq[: 2 * 20 * Q])[0], rx.run(iq[2 * 20 * Q:])[0]])
    assert not np.array_equal(bits_f32(bare), bits_f32(whole))
    m = tm.TunerModel(tm.FS, 1.0)
    m.add(0, 0, IFS[2], 128_000, tm.CHAN_RATE, USB, tm.AUDIO_PASSBAND, tm.CHAN_RATE // D2)
    got = []
    for a, b in ((0, 20), (20, 32)):
        m.submit(iq[2 * a * Q: 2 * b * Q])
        got.append(m.audio(0))
    assert np.array_equal(bits_f32(np.concatenate(got)), bits_f32(whole))
