"""-m gpu: a tuner's getters and controls used together, the way a caller between blocks would -- random scripts of submits,
setters, receivers coming and going, seeks and every getter (tests/tuner_model.py: make_script), played on a wr_tuner and on
the CPU model of one (TunerModel: the oracle's receivers and the numpy restatements of squelch, AGC, levels and tone bank).

  test_script_against_the_model      WR_NCO_EXACT, a launch per block: whatever an operation hands back is the model's
  test_script_in_every_launch_mode   WR_NCO_ROTATE: a launch per block, held blocks and the streaming launch hand back the
                                     same bits, and the first of them is the model's within the ROTATE tolerance
  test_a_receiver_leaves_between_a_submit_and_its_pushes      the rows of a tuner push are counted when the push is made
  test_setters_between_a_submit_and_its_pushes                 staged setters wait for the next block, the voice word does not
  test_a_receiver_moves_to_another_rate_group_and_back
  test_caller_designed_taps          wr_chan_set_taps(_n) with taps of full size at every position

The scripts play the resampler, the DCS bank and the voice bank (with a second resampler behind it) as well: GpuPlay pushes
first and only then downloads the tuner's rows, so that the push is what flushes; every push is compared with the model and,
on every live row, with the restatement fed the library's own rows.

Tolerances are the suite's own: DB_ATOL on bins within 60 dB of a row's peak (speccases.db_error), FM_ATOL and the ROTATE
bound through the audio filter's absolute gain, IQ_ATOL on ROTATE channel IQ (tunercases.py)."""
import ctypes as C

import numpy as np
import pytest

import agc_np
import rowcases
import tuner_model as tm
from speccases import DB_ATOL, db_error
from tunercases import IQ_ATOL, LINEAR_ATOL, OracleChain, bits_f32
from webradio_amd import capi
from webradio_amd.device import Resampler, Spectrum, ToneBank, Tuner, VoiceBank

pytestmark = pytest.mark.gpu

CPB, APB = tm.CHAN_PASSBANDS[0], tm.AUDIO_PASSBAND
WR_TUNE_DDC_NG2_MIN_PASSES = 1                                            # include/webradio_amd.h: enum wr_tunable


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32 or b.dtype == np.float32:
        return np.array_equal(bits_f32(a), bits_f32(b))
    return np.array_equal(a, b)


def _same(a, b):
    """two results of an operation, bit for bit, whatever their shape"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return _same_bits(a, b)


class GpuPlay:
    """a script's operations on a wr_tuner; do(op) returns what ModelPlay.do returns for it, from the library"""

    def __init__(self, dev, script, iq, x, nco, how="block"):
        self.dev, self.s, self.iq, self.x = dev, script, iq, x
        s = script
        self.t = t = Tuner(dev, tm.FS, s["max_channels"], s["max_block"], nco)
        for c, f in enumerate(s["ifs"]):
            assert t.add_receiver(f, CPB, tm.CHAN_RATE, c % 4, APB, s["audio_rate"]) == c and t.slot(c) == c
        capi.check(t.lib.wr_tuner_set_audio_scale(t.h, C.c_float(s["scale"])))
        t.audio_ring(128)
        if how == "hold":
            t.blocks_per_launch(s["hold"])
        if how == "stream":
            t.streaming(True)
        self.rows = tm.slot_rows(s["max_channels"])
        steps = tm.bank_steps(s["audio_rate"])
        self.banks = [ToneBank(dev, self.rows, None, None, w, steps=steps) for w in tm.BANK_WINDOWS]
        self.chan_spec = Spectrum(dev, tm.CHAN_SPECTRUM_N)
        self.audio_spec = Spectrum(dev, tm.AUDIO_SPECTRUM_N, real=True)
        self.live = {c: c for c in range(s["nrx"])}                       # handle -> slot
        self.pos = 0
        self.cap = s["max_block"] // tm.D1
        # the row banks (tm.bank_shapes), their outputs a few floats wider than the longest row, and the restatements that are
        # fed the library's own rows: under WR_NCO_ROTATE, where the model's audio is only close, they hold the banks
        shapes, k2max = tm.bank_shapes(s), self.cap // s["d2"]
        self.resamp = Resampler(dev, self.rows, 4, 3, taps=shapes["resamp"][2])
        self.chain = Resampler(dev, self.rows, 3, 4, taps=shapes["chain"][2])
        assert (self.resamp.L, self.resamp.M, self.chain.L, self.chain.M) == (3, 4, 4, 3)
        self.voice = VoiceBank(dev, self.rows, shapes["voice"])
        self.voice.set_rows(0, np.arange(self.rows) % tm.VOICE_FILTERS)
        self.dcs = rowcases.dcs_bank(dev, self.rows, shapes["words"], tm.DCS_STEP, tm.DCS_MAX_ERRORS)
        self.out = {"resamp": rowcases.OutRows(dev, self.rows, (3 * k2max + 3) // 4 + 1 + 5),
                    "voice": rowcases.OutRows(dev, self.rows, k2max + 3),
                    "chain": rowcases.OutRows(dev, self.rows, (4 * k2max + 2) // 3 + 1 + 6)}
        self.rb = tm.RowBanks(s)
        self.seen = {k: 0 for k in tm.BANK_KINDS}                         # rows held to the restatement, refusals, words set

    def close(self):
        for b in self.banks + [self.resamp, self.chain, self.voice, self.dcs]:
            b.destroy()
        for o in self.out.values():
            o.free()
        self.chan_spec.destroy()
        self.audio_spec.destroy()
        self.t.destroy()

    def bank(self, b):
        iq, energy, windows, fill = self.banks[b].read()
        return {s: (iq[s].copy(), int(energy[s]), int(windows[s]), int(fill[s])) for s in self.live.values()}

    def _own_rows(self, slots, what):
        """the library's own rows of the last submit, for the restatements; asked for BEHIND the push, so that the push and
        not this download is what sends held blocks out and closes an open streaming launch"""
        rows = self.t.fetch_audio_all()
        assert rows.shape[0] == slots >= max(self.live.values()) + 1, (what, rows.shape, slots)
        return rows

    def _held(self, kind, got, want, what):
        """every live row bit for bit, FM receivers and AGC rows included"""
        assert got.shape == want.shape, (what, got.shape, want.shape)
        for s in self.live.values():
            assert rowcases.same_bits(got[s], want[s]), (what, s)
        self.seen[kind] += len(self.live)

    def _push(self, kind, what):
        t, lib = self.t, self.t.lib
        slots, n_out = C.c_uint(), C.c_size_t()
        if kind == "resamp":
            out = self.out["resamp"]
            capi.check(lib.wr_tuner_resamp_push(t.h, self.resamp.h, C.c_void_p(out.p), out.stride, C.byref(n_out), C.byref(slots)))
            got = out.take(slots.value, n_out.value, what)
            self._held(kind, got, self.rb.push_resamp(self._own_rows(slots.value, what)), what)
            assert self.resamp.info()[3:] == self.rb.counts("resamp"), what
            return n_out.value, {s: got[s] for s in self.live.values()}
        if kind == "dcs":
            capi.check(lib.wr_tuner_dcs_push(t.h, self.dcs.h, C.byref(slots)))
            got, want = self.dcs.read(), self.rb.push_dcs(self._own_rows(slots.value, what))
            for s in self.live.values():
                assert all(np.array_equal(g[s], w[s]) for g, w in zip(got, want)), (what, s, got[3][s], want[3][s])
            self.seen[kind] += len(self.live)
            assert self.dcs.info()[3:] == self.rb.counts("dcs"), what
            return tm.dcs_by_slot(got, self.live.values())
        out, then = self.out["voice"], self.out["chain"]
        capi.check(lib.wr_tuner_voice_push(t.h, self.voice.h, C.c_void_p(out.p), out.stride, C.byref(slots)))
        rows = self._own_rows(slots.value, what)
        k2 = rows.shape[1]
        # the output block goes straight on into the second resampler, as a caller chains them
        n = self.chain.push_rows(out.p, out.stride, slots.value, k2, then.p, then.stride)
        y, z = out.take(slots.value, k2, what), then.take(slots.value, n, what)
        want_y, want_z = self.rb.push_voice(rows)
        self._held(kind, y, want_y, what)
        self._held(kind, z, want_z, what)
        assert (self.voice.info()[2],) + self.chain.info()[3:] == self.rb.counts("voice"), what
        return {s: y[s] for s in self.live.values()}, n, {s: z[s] for s in self.live.values()}

    def _push_again(self, kind, what):
        """the same submit pushed twice: WR_ERR_STATE, nothing written, nothing counted"""
        t, lib = self.t, self.t.lib
        n_out = C.c_size_t()
        if kind == "resamp":
            out = self.out["resamp"]
            rc = lib.wr_tuner_resamp_push(t.h, self.resamp.h, C.c_void_p(out.p), out.stride, C.byref(n_out), None)
        elif kind == "dcs":
            rc = lib.wr_tuner_dcs_push(t.h, self.dcs.h, None)
        else:
            out = self.out["voice"]
            rc = lib.wr_tuner_voice_push(t.h, self.voice.h, C.c_void_p(out.p), out.stride, None)
        assert rc == capi.WR_ERR_STATE and b"already" in lib.wr_last_error(), (what, rc, lib.wr_last_error())
        self.seen[kind + "_again"] += 1
        if kind == "dcs":
            return self.dcs.info()[3:], tm.dcs_by_slot(self.dcs.read(), self.live.values())
        out.peek(0, 0, what)
        return self.resamp.info()[3:] if kind == "resamp" else (self.voice.info()[2],) + self.chain.info()[3:]

    def do(self, op):
        t, k, lib = self.t, op[0], self.t.lib
        what = (self.s["seed"], op)
        if k in tm.PUSH_KINDS:
            return self._push(k, what)
        if k.endswith("_again") and k != "tones_again":
            return self._push_again(k[:-6], what)
        if k == "voice_ctl":
            self.voice.set_rows(op[1], [op[2]])
            self.rb.voice.set_rows(op[1], [op[2]])
            self.seen[k] += 1
        elif k == "submit":
            if op[1] == "host":
                t.submit_host(self.iq[2 * self.pos: 2 * (self.pos + op[2])])
            else:
                t.submit_device(self.x + 8 * self.pos, op[2])
            self.pos += op[2]
        elif k == "set_if":
            t.set_if(op[1], op[2])
        elif k == "set_mode":
            t.set_mode(op[1], op[2])
        elif k == "set_filter":
            t.set_filter(op[1], 0, op[2], tm.CHAN_RATE)
        elif k == "af_gain":
            t.set_af_gain(op[1], op[2])
        elif k in ("squelch_on", "squelch_thr"):
            t.set_squelch(op[1], op[2], True)
        elif k == "squelch_off":
            t.set_squelch(op[1], 0.0, False)
        elif k in ("agc_on", "agc_new"):
            t.set_agc(op[1], *op[2])
        elif k == "agc_off":
            t.set_agc(op[1], enable=False)
        elif k == "reset_history":
            capi.check(lib.wr_chan_reset_history(t.h, op[1]))
        elif k == "seek":
            t.seek(op[1])
        elif k == "remove":
            t.remove_receiver(op[1])
            del self.live[op[1]]
        elif k == "add":
            c = t.add_receiver(op[3], CPB, tm.CHAN_RATE, op[4], APB, self.s["audio_rate"])
            assert (c, t.slot(c)) == (op[1], op[2]), (op, c, t.slot(c))   # the lowest free handle, the slot that was left
            self.live[c] = op[2]
        elif k == "bank_reset":
            for b in self.banks + [self.resamp, self.chain, self.voice]:
                b.reset(op[1])
            if op[1] >= 0 or self.s["seed"] % 2 == 0:
                self.dcs.reset(op[1])
            else:                                                         # the bank joins the stream where the seek put it
                self.dcs.seek(tm.audio_pos(self.s, self.pos))
            self.rb.reset(op[1], self.pos)
            assert np.array_equal(self.voice.get_rows(), self.rb.voice.ctl), what     # the control words survive a reset
        elif k == "fetch_audio":
            return t.fetch(op[1], capi.WR_STAGE_AUDIO, self.cap)
        elif k == "fetch_chan":
            return t.fetch(op[1], capi.WR_STAGE_CHAN_IQ, 2 * self.cap)
        elif k == "fetch_all":
            rows = t.fetch_audio_all()
            return {s: rows[s].copy() for s in self.live.values()}
        elif k == "levels":
            mean, peak, muted, frames, audio_frames = t.chan_levels()
            return {c: (mean[s], peak[s], int(muted[s])) for c, s in self.live.items()}, frames, audio_frames
        elif k == "spectra":
            rows = t.chan_spectra(self.chan_spec, op[1])
            return {c: rows[s].copy() for c, s in self.live.items()}
        elif k == "audio_spectrum":
            a, stride, frames = t.audio_dev()
            assert frames >= tm.AUDIO_SPECTRUM_N
            n, used = tm.AUDIO_SPECTRUM_N, max(self.live.values()) + 1
            out = self.dev.malloc(used * n * 4)
            try:
                self.audio_spec.batch_db_rows(a, stride, used, out)
                self.dev.sync()
                rows = self.dev.download(out, used * n).reshape(used, n)
            finally:
                self.dev.free(out)
            return {c: rows[s].copy() for c, s in self.live.items()}
        elif k == "tones":
            assert t.tones_push(self.banks[op[1]]) >= max(self.live.values()) + 1
            return self.bank(op[1])
        elif k == "tones_again":
            assert lib.wr_tuner_tones_push(t.h, self.banks[op[1]].h, None) == capi.WR_ERR_STATE     # ... and nothing is counted
            assert b"already" in lib.wr_last_error()
            return self.bank(op[1])
        elif k == "get_agc":
            return t.get_agc(op[1])
        elif k == "state":
            return t.state(op[1])[0]
        elif k == "flush":
            t.flush()
        elif k == "drain":
            out = []
            while t.ring_stats()[0]:
                rows, seq = t.ring_acquire()
                whole = np.zeros((self.rows, rows.shape[1]), np.float32)  # (an entry holds the lane groups in use)
                whole[: rows.shape[0]] = rows
                out.append((seq, whole))
                t.ring_release()
            return out
        return None


@pytest.fixture(scope="module")
def scripts(dev):
    """scripts(seed) -> (script, the stream on the host, the stream in device memory); made once per seed"""
    made = {}

    def get(seed):
        if seed not in made:
            script = tm.make_script(seed)
            iq = tm.signal(script["total"], script["carriers"], seed)
            made[seed] = (script, iq, dev.upload(iq))
        return made[seed]
    yield get
    dev.sync()
    for _, _, x in made.values():
        dev.free(x)


# ---- 1: every operation's answer against the model --------------------------------------------------------------------------

def _audio_is_the_models(m, c, got, want, what):
    """bit for bit; a receiver that has run the FM detector since its histories were last empty: within the FM tolerance"""
    r = m.rxs[c]
    assert got.shape == want.shape, what
    if not r.was_fm:
        bad = np.flatnonzero(bits_f32(got) != bits_f32(want))
        assert bad.size == 0, (what, c, bad[:4], got[bad[:4]], want[bad[:4]])
        return 1
    if not r.used_agc and want.size:
        assert float(np.abs(got - want).max()) <= m.fm_tolerance(c), (what, c)
    return 0


def _of_slot(result, slot):
    """what a bank operation's result says of one slot: the {slot: ...} dicts in it cut down to that slot"""
    if isinstance(result, dict):
        return result[slot]
    if isinstance(result, (tuple, list)):
        return tuple(_of_slot(x, slot) for x in result)
    return result


def _check_exact(play, op, got, want, seen):
    m, k = play.m, op[0]
    by_slot = {r.slot: c for c, r in m.rxs.items()}
    what = (play.s["seed"], k, op[1:] if k != "add" else op[1])
    if k == "fetch_audio":
        seen["exact"] += _audio_is_the_models(m, op[1], got, want, what)
    elif k == "fetch_chan":
        assert _same_bits(got, want), what
    elif k == "fetch_all":
        assert got.keys() == want.keys(), what
        for s in got:
            seen["exact"] += _audio_is_the_models(m, by_slot[s], got[s], want[s], what)
    elif k == "drain":
        assert [seq for seq, _ in got] == [e[0] for e in want], what
        for (seq, rows), (_, audio, standing) in zip(got, want):
            for s, w in audio.items():                                    # (the receiver's standing when the block was made)
                exact, tol, _ = standing[s]
                assert rows[s].shape == w.shape, (what, seq, s)
                if exact:
                    assert _same_bits(rows[s], w), (what, seq, s)
                elif tol is not None and w.size:
                    assert float(np.abs(rows[s] - w).max()) <= tol, (what, seq, s)
                seen["exact"] += exact
    elif k == "levels":
        assert _same(got, want), (what, [c for c in want[0] if not _same(got[0][c], want[0][c])][:4], got[1:], want[1:])
    elif k == "spectra":
        assert got.keys() == want.keys()
        for c in got:
            assert db_error(got[c], want[c]) <= DB_ATOL, (what, c)
    elif k == "audio_spectrum":
        for c in got:
            if not m.rxs[c].was_fm and float(np.abs(m.audio(c)[: tm.AUDIO_SPECTRUM_N]).max()) > 0.0:
                assert db_error(got[c], want[c]) <= DB_ATOL, (what, c)
    elif k in ("tones", "tones_again"):
        for c, r in m.rxs.items():
            if not r.was_fm:
                assert _same(got[r.slot], want[r.slot]), (what, c, got[r.slot][1:], want[r.slot][1:])
                seen["latched"] += want[r.slot][2] > 0
    elif k in tm.BANK_KINDS and k != "voice_ctl":
        # the rule `tones` uses: bit for bit on every row whose receiver has not run the FM detector; the frame counts always
        for c, r in m.rxs.items():
            if not r.was_fm:
                assert _same(_of_slot(got, r.slot), _of_slot(want, r.slot)), (what, c)
                seen[k] += 1
    elif k == "get_agc":
        assert _same(got, want), (what, got, want)
        seen["agc"] += bool(want[0])
    elif k == "state":
        assert got == want, what


@pytest.mark.parametrize("seed", tm.fuzz_seeds())
def test_script_against_the_model(dev, scripts, seed):
    script, iq, x = scripts(seed)
    model, gpu = tm.ModelPlay(script, iq), GpuPlay(dev, script, iq, x, capi.WR_NCO_EXACT)
    seen = {"exact": 0, "gated": 0, "latched": 0, "agc": 0}
    seen.update({k: 0 for k in tm.BANK_KINDS if k != "voice_ctl"})
    try:
        for op in script["ops"]:
            got, want = gpu.do(op), model.do(op)
            assert (got is None) == (want is None), op
            if want is not None:
                _check_exact(model, op, got, want, seen)
            if op[0] == "submit":                                         # a squelch that closes and opens within the block
                seen["gated"] += any(0 < r.gate()[0] < r.last[3] for r in model.m.rxs.values() if r.used_sq is not None)
        for c in gpu.live:                                                # the NCO phases at the end
            assert gpu.t.state(c)[0] == model.m.phase(c), c
        assert gpu.live == {c: r.slot for c, r in model.m.rxs.items()}
        assert gpu.t.agc_info()[0] == model.m.agc_on()
    finally:
        gpu.close()
    print("seed %d: held to the model %s, to the restatement on the library's rows %s" % (seed, seen, gpu.seen))
    assert seen["exact"] > 0 and seen["latched"] > 0 and seen["gated"] > 0 and seen["agc"] > 0
    assert not [k for k in tm.PUSH_KINDS if seen[k] < 1 or gpu.seen[k] < 1], (seen, gpu.seen)


# ---- 2: a launch per block, held blocks, the streaming launch -------------------------------------------------------------------

def _ring_mask(script, rows):
    """[rows][audio frames of the whole script]: where a receiver sat in the slot when the frame was made"""
    live = {c: c for c in range(script["nrx"])}
    parts = []
    for op in script["ops"]:
        if op[0] == "remove":
            del live[op[1]]
        elif op[0] == "add":
            live[op[1]] = op[2]
        elif op[0] == "submit":
            m = np.zeros((rows, op[2] // tm.D1 // script["d2"]), bool)
            m[sorted(live.values())] = True
            parts.append(m)
    return np.concatenate(parts, axis=1)


def _check_rotate(model, op, got, want, ring):
    """the play with a launch per block against the model: audio of receivers that never ran the FM detector and have neither
    AGC nor squelch in use, within the ROTATE tolerance through the audio filter (test_gpu_fuzz.py); `ring`: the model's
    entries the library has not handed out yet (a block's entry may wait for the next submit: wr_tuner_flush)"""
    m, k = model.m, op[0]
    pairs = []
    if k == "drain":
        ring.update({seq: (audio, standing) for seq, audio, standing in want})
        n = 0
        for seq, rows in got:
            audio, standing = ring.pop(seq)
            for s, w in audio.items():
                if standing[s][2] is not None and w.size:
                    assert rows[s].shape == w.shape and float(np.abs(rows[s] - w).max()) <= standing[s][2], (op, seq, s)
                    n += 1
        return n
    if k == "fetch_audio":
        pairs = [(op[1], got, want)]
    elif k == "fetch_all":
        by_slot = {r.slot: c for c, r in m.rxs.items()}
        pairs = [(by_slot[s], got[s], want[s]) for s in want]
    elif k == "fetch_chan":
        assert float(np.abs(got - want).max()) <= IQ_ATOL, op             # (ROTATE channel IQ)
    n = 0
    for c, g, w in pairs:
        r = m.rxs[c]
        if c % 4 != 1 and not r.used_agc and r.used_sq is None and w.size:
            assert g.shape == w.shape and float(np.abs(g - w).max()) <= m.rotate_tolerance(c), (op, c)
            n += 1
    return n


@pytest.mark.parametrize("seed", tm.fuzz_seeds())
def test_script_in_every_launch_mode(dev, scripts, seed):
    script, iq, x = scripts(seed)
    lib = dev.lib
    previous = C.c_long()
    ng2 = script["nrx"] == 128                   # two full lane groups: the script runs under the two-lane-group kernel
    if ng2:
        assert lib.wr_tune(WR_TUNE_DDC_NG2_MIN_PASSES, C.c_long(0), C.byref(previous)) == 0
    try:
        plays, held_to_model, model_ring = {}, 0, {}
        for how in ("block", "hold", "stream"):
            gpu = GpuPlay(dev, script, iq, x, capi.WR_NCO_ROTATE, how)
            model = tm.ModelPlay(script, iq) if how == "block" else None
            results, ring = [], []
            try:
                for op in script["ops"]:
                    got = gpu.do(op)
                    if model is not None:
                        held_to_model += _check_rotate(model, op, got, model.do(op), model_ring)
                    if op[0] == "drain":
                        ring += [rows for _, rows in got]
                    else:
                        results.append(got)
                assert gpu.t.ring_stats() == (0, 0)
                plays[how] = (results, np.concatenate(ring, axis=1), gpu.t.stream_info(), gpu.t.agc_info())
                print("seed %d, %s: rows held to the restatement on the library's rows %s" % (seed, how, gpu.seen))
                assert not [k for k in tm.PUSH_KINDS if gpu.seen[k] < 1], (how, gpu.seen)
            finally:
                gpu.close()
    finally:
        if ng2:
            assert lib.wr_tune(WR_TUNE_DDC_NG2_MIN_PASSES, C.c_long(previous.value), None) == 0
    assert held_to_model > 0 and not model_ring                           # every block's ring entry was held to the model's
    base, ring, _, agc = plays["block"]
    mask = _ring_mask(script, ring.shape[0])
    assert mask.shape == ring.shape and ring.shape[1] > 0
    for how in ("hold", "stream"):
        results, other_ring, info, other_agc = plays[how]
        for i, (a, b) in enumerate(zip(base, results)):
            assert _same(a, b), (how, i, [op for op in script["ops"] if op[0] != "drain"][i])
        assert other_ring.shape == ring.shape, how
        assert np.array_equal(bits_f32(ring)[mask], bits_f32(other_ring)[mask]), how
        assert other_agc == agc, how
    print("seed %d: stream_info %s, agc_info %s, %d audio rows held to the model" % (seed, plays["stream"][2], agc, held_to_model))
    assert plays["stream"][2][2] >= 3                                     # blocks that did stream
    assert plays["block"][2][2] == 0 and plays["hold"][2][2] == 0


# ---- 2a: between a submit and its pushes ------------------------------------------------------------------------------------------

class _FourBanks:
    """the four row banks of `rows` rows behind a tuner at 1 kHz audio, each with its restatement; push(t) pushes the last
    submit into all of them, feeds the restatements the library's own rows and compares EVERY row of the banks"""

    def __init__(self, dev, rows, seed=0):
        script = {"seed": seed, "audio_rate": 1_000, "max_channels": rows, "d2": 5}
        shapes = tm.bank_shapes(script)
        self.dev, self.rows, self.rb = dev, rows, tm.RowBanks(script)
        self.resamp = Resampler(dev, rows, 4, 3, taps=shapes["resamp"][2])
        self.voice = VoiceBank(dev, rows, shapes["voice"])
        self.voice.set_rows(0, np.arange(rows) % tm.VOICE_FILTERS)
        self.dcs = rowcases.dcs_bank(dev, rows, shapes["words"], tm.DCS_STEP, tm.DCS_MAX_ERRORS)
        self.tones = ToneBank(dev, rows, None, None, 16, steps=tm.bank_steps(1_000)[:2])
        self.want_tones = tm.tones_np.Bank(rows, tm.bank_steps(1_000)[:2], 16)
        self.out = {"resamp": rowcases.OutRows(dev, rows, 64), "voice": rowcases.OutRows(dev, rows, 64)}

    def close(self):
        for b in (self.resamp, self.voice, self.dcs, self.tones):
            b.destroy()
        for o in self.out.values():
            o.free()

    def reset(self, row):
        for b in (self.resamp, self.voice, self.dcs, self.tones, self.want_tones):
            b.reset(row)
        self.rb.reset(row, 0)

    def check(self, y, want_y, v, want_v, what):
        assert rowcases.same_bits(y, want_y) and rowcases.same_bits(v, want_v), what
        for g, w in zip(self.dcs.read(), self.rb.read_dcs()):
            assert np.array_equal(g, w), what
        for g, w in zip(self.tones.read(), self.want_tones.read()):
            assert np.array_equal(g, w), what

    def push(self, t, what):
        """-> (slots, the library's own rows, the resampler's frames, the voice bank's frames)"""
        lib, slots, n_out, counted = t.lib, C.c_uint(), C.c_size_t(), []
        o = self.out["resamp"]
        capi.check(lib.wr_tuner_resamp_push(t.h, self.resamp.h, C.c_void_p(o.p), o.stride, C.byref(n_out), C.byref(slots)))
        counted.append(slots.value)
        y = o.take(slots.value, n_out.value, what)
        o = self.out["voice"]
        capi.check(lib.wr_tuner_voice_push(t.h, self.voice.h, C.c_void_p(o.p), o.stride, C.byref(slots)))
        counted.append(slots.value)
        capi.check(lib.wr_tuner_dcs_push(t.h, self.dcs.h, C.byref(slots)))
        counted.append(slots.value)
        counted.append(t.tones_push(self.tones))
        rows = t.fetch_audio_all()
        assert counted == [rows.shape[0]] * 4, (what, counted, rows.shape)
        v = o.take(rows.shape[0], rows.shape[1], what)
        self.rb.dcs.push(rows)
        self.want_tones.push(rows)
        self.check(y, self.rb.push_resamp(rows), v, self.rb.voice.push(rows), what)
        return rows.shape[0], rows, y, v

    def push_plain(self, v, what):
        """plain rows into the resampler and the voice bank: what every row's history holds shows in what comes out"""
        p = rowcases.upload_rows(self.dev, v, v.shape[1] + 3)
        try:
            o = self.out["resamp"]
            n = self.resamp.push_rows(p, v.shape[1] + 3, v.shape[0], v.shape[1], o.p, o.stride)
            y = o.take(v.shape[0], n, what)
            o = self.out["voice"]
            self.voice.push_rows(p, v.shape[1] + 3, v.shape[0], v.shape[1], o.p, o.stride)
            self.check(y, self.rb.push_resamp(v), o.take(v.shape[0], v.shape[1], what), self.rb.voice.push(v), what)
        finally:
            self.dev.free(p)


@pytest.mark.parametrize("how", ["block", "hold", "stream"])
def test_a_receiver_leaves_between_a_submit_and_its_pushes(dev, how):
    """The rows of a tuner push are counted when the push is made (wr_tuner_tones_push in the header), not when the submit
    was.  65 receivers: the 65th sits alone in the second lane group.  Two blocks go into all four banks with 128 rows; after
    the third submit the 65th is removed, and the pushes of that submit count 64 slots: the resampler, the DCS bank and the
    voice bank reset the rows a push leaves out -- plain rows pushed next come out of empty histories in rows 64 ... -- and
    the tone bank keeps them.  The receiver then comes back into slot 64, the caller resets that row, and two more blocks
    agree with the restatements in every row."""
    nrx, n = 65, 20 * tm.D1 * 5
    ifs = tm._ifs(nrx)
    modes = [(tm.AM, tm.USB, tm.LSB)[c % 3] for c in range(nrx)]
    iq = tm.signal(5 * n, [ifs[3], ifs[64]], seed=11)
    x = dev.upload(iq)
    t = Tuner(dev, tm.FS, nrx, 2 * n, capi.WR_NCO_EXACT)
    banks = _FourBanks(dev, 128)
    try:
        for c in range(nrx):
            assert t.add_receiver(ifs[c], CPB, tm.CHAN_RATE, modes[c], APB, 1_000) == c and t.slot(c) == c
        if how == "hold":
            t.blocks_per_launch(2)
        if how == "stream":
            t.streaming(True)
        for b in range(2):
            t.submit_device(x + 8 * n * b, n)
            slots, rows, _, _ = banks.push(t, (how, b))
            assert slots == 128 and float(np.abs(rows[64]).max()) > 0.0
        kept = [a[64].copy() for a in banks.tones.read()]
        assert int(kept[2]) == 2 and int(kept[3]) == 8                    # 40 frames: two windows of 16 and 8 in the open one
        assert int(banks.dcs.read()[3][64]) >= 1
        t.submit_device(x + 8 * n * 2, n)
        t.remove_receiver(64)                                             # ... between the submit and its pushes
        slots, rows, _, _ = banks.push(t, (how, "left"))
        assert slots == 64 and rows.shape == (64, 20)
        assert not any(a[64:].any() for a in banks.dcs.read())            # reset: the resampler's convention
        assert all(np.array_equal(a[64], k) for a, k in zip(banks.tones.read(), kept))     # ... which the tone bank does not have
        banks.push_plain(rowcases.special_rows(128, 9, 12, 3, [1.0, -0.0]), (how, "plain"))
        assert t.add_receiver(ifs[64], CPB, tm.CHAN_RATE, modes[64], APB, 1_000) == 64 and t.slot(64) == 64
        banks.reset(64)
        for b in (3, 4):
            t.submit_device(x + 8 * n * b, n)
            slots, rows, _, _ = banks.push(t, (how, b))
            assert slots == 128 and float(np.abs(rows[64]).max()) > 0.0
    finally:
        banks.close()
        t.destroy()
        dev.free(x)


def test_setters_between_a_submit_and_its_pushes(dev):
    """wr_chan_set_af_gain and wr_chan_set_mode issued behind a submit are staged: the pushes of that submit still take its
    audio, and the next block has the new settings.  wr_voice_set_rows issued there applies with this push, as its header
    says.  Five receivers, none FM, WR_NCO_EXACT: every row is the model's bit for bit."""
    nrx, n = 5, 20 * tm.D1 * 5
    ifs = tm._ifs(nrx)
    modes = [tm.AM, tm.USB, tm.LSB, tm.AM, tm.USB]
    iq = tm.signal(3 * n, [ifs[0], ifs[3]], seed=13)
    t = Tuner(dev, tm.FS, nrx, n, capi.WR_NCO_EXACT)
    m, twin = tm.TunerModel(tm.FS, 1.0), tm.TunerModel(tm.FS, 1.0)        # twin: no setter ever reaches it
    banks = _FourBanks(dev, 64, seed=1)
    want = tm.RowBanks(banks.rb.script)                                   # ... fed the model's rows
    try:
        for c in range(nrx):
            assert t.add_receiver(ifs[c], CPB, tm.CHAN_RATE, modes[c], APB, 1_000) == c
            for model in (m, twin):
                model.add(c, c, ifs[c], CPB, tm.CHAN_RATE, modes[c], APB, 1_000)
        for b in range(3):
            block = iq[2 * n * b: 2 * n * (b + 1)]
            t.submit_host(block)
            m.submit(block)
            twin.submit(block)
            if b == 1:                                                    # behind the submit, in front of its pushes
                t.set_af_gain(0, 6.0)
                m.set_af_gain(0, 6.0)
                t.set_mode(1, tm.LSB)
                m.set_mode(1, tm.LSB)
                for bank in (banks.voice, banks.rb.voice, want.voice):
                    bank.set_rows(2, [1 | VoiceBank.MUTE, 1])             # row 2 muted, row 3 on another filter
            slots, rows, y, v = banks.push(t, b)
            assert slots == 64
            for c in range(nrx):
                assert _same_bits(rows[c], m.audio(c)), (b, c)
            mine = m.audio_rows(64)
            assert _same_bits(y[:nrx], want.push_resamp(mine)[:nrx]) and _same_bits(v[:nrx], want.push_voice(mine)[0][:nrx]), b
            changed = [c for c in range(nrx) if not _same_bits(m.audio(c), twin.audio(c))]
            assert changed == ([0, 1] if b == 2 else []), (b, changed)    # staged: the next block has them, this one does not
            if b >= 1:
                assert not v[2].any() and v[3].any()
                other = tm.voice_np.Bank(1, banks.voice.taps[0])
                assert not _same_bits(v[3], other.push(rows[3:4])[0])     # (filter 0 on an empty history would say something else)
    finally:
        banks.close()
        t.destroy()


# ---- 3: a receiver moves to another rate group and back -------------------------------------------------------------------------

def test_a_receiver_moves_to_another_rate_group_and_back(dev):
    """wr_chan_set_filter on stage 1 with another audio rate seats the receiver in a rate group of its own; the same call with
    the old rate brings it back into the slot it left.  Either way it arrives like a new receiver -- empty filter histories,
    its AGC from floor with a step for the rate it now has -- except for the NCO phase and the detector's previous frame; the
    other receivers never lose a bit.  While there are two rate groups the per-tuner getters answer WR_ERR_STATE."""
    lib = dev.lib
    nrx, n, mover = 6, 80 * tm.D1, 2
    ifs = [(c - 3) * 25_000 + 321 for c in range(nrx)]
    modes = [tm.AM, tm.FM, tm.USB, tm.LSB, tm.AM, tm.USB]
    settings = (-12.0, 5.0, 60.0)
    iq = tm.signal(7 * n, [ifs[0], ifs[mover]], seed=5)
    t = Tuner(dev, tm.FS, nrx, n, capi.WR_NCO_EXACT)
    m, twin = tm.TunerModel(tm.FS, 1.0), tm.TunerModel(tm.FS, 1.0)        # twin: the receiver never moves
    for c in range(nrx):
        assert t.add_receiver(ifs[c], CPB, tm.CHAN_RATE, modes[c], APB, 1_000) == c
        for model in (m, twin):
            model.add(c, t.slot(c), ifs[c], CPB, tm.CHAN_RATE, modes[c], APB, 1_000)
    for c in (mover, 4):
        t.set_agc(c, *settings)
    t.set_squelch(0, -46.0, True)
    t.set_af_gain(3, 6.0)
    for model in (m, twin):
        model.set_agc(mover, settings)
        model.set_agc(4, settings)
        model.set_squelch(0, -46.0)
        model.set_af_gain(3, 6.0)
    bank = ToneBank(dev, 64, None, None, 16, steps=tm.bank_steps(1_000))
    want_bank = tm.tones_np.Bank(64, tm.bank_steps(1_000), 16)
    spec = Spectrum(dev, tm.CHAN_SPECTRUM_N)
    out = dev.malloc(64 * tm.CHAN_SPECTRUM_N * 4)
    pos = [0]

    def block(one_group):
        b = iq[2 * pos[0]: 2 * (pos[0] + n)]
        pos[0] += n
        t.submit_host(b)
        m.submit(b)
        twin.submit(b)
        for c in range(nrx):
            k1 = n // tm.D1
            assert _same_bits(t.fetch(c, capi.WR_STAGE_CHAN_IQ, 2 * k1), m.chan_iq(c)), (pos[0] // n, c)
            ga, wa = t.fetch(c, capi.WR_STAGE_AUDIO, k1), m.audio(c)
            if modes[c] == tm.FM:
                assert ga.shape == wa.shape and float(np.abs(ga - wa).max()) <= m.fm_tolerance(c)
            else:
                assert _same_bits(ga, wa), (pos[0] // n, c)
            got = t.get_agc(c)
            assert _same(got, m.get_agc(c)), (pos[0] // n, c, got, m.get_agc(c))
        if not one_group:
            assert lib.wr_tuner_chan_levels(t.h, capi.ptr(np.zeros(64, np.float32)), None, None, None, None, None) == capi.WR_ERR_STATE
            assert b"several rate groups" in lib.wr_last_error()
            assert lib.wr_tuner_chan_spectra(t.h, spec.h, 0, C.c_void_p(out), None) == capi.WR_ERR_STATE
            assert b"several rate groups" in lib.wr_last_error()
            assert lib.wr_tuner_tones_push(t.h, bank.h, None) == capi.WR_ERR_STATE
            assert b"several rate groups" in lib.wr_last_error()
            return
        mean, peak, muted, frames, audio_frames = t.chan_levels()
        rows = t.chan_spectra(spec, 7)
        assert t.tones_push(bank) == 64
        want_bank.push(m.audio_rows(64))
        got_bank, ref_bank = bank.read(), want_bank.read()
        assert (frames, audio_frames) == (n // tm.D1, n // tm.D1 // 5)
        for c in range(nrx):
            s = t.slot(c)
            assert _same((mean[s], peak[s], int(muted[s])), m.levels(c)), (pos[0] // n, c)
            assert db_error(rows[s], m.chan_spectrum(c, 7)) <= DB_ATOL, (pos[0] // n, c)
            if modes[c] != tm.FM:
                for g, w in zip(got_bank, ref_bank):
                    assert np.array_equal(g[s], w[s]), (pos[0] // n, c)

    try:
        block(True)
        block(True)
        home = t.slot(mover)
        carried = t.get_agc(mover)[4]
        floor_bits = agc_np.design(*settings, 1_000)[1]
        assert carried > floor_bits                                       # an envelope that a reset would be seen to lose
        t.set_filter(mover, 1, APB, 2_500)                                # 5 kHz -> 2.5 kHz: a rate group of its own
        m.set_audio_rate(mover, APB, 2_500, t.slot(mover))
        block(False)
        assert t.get_agc(mover)[3] == agc_np.design(*settings, 2_500)[2] != agc_np.design(*settings, 1_000)[2]
        block(False)
        assert t.fetch(mover, capi.WR_STAGE_AUDIO, n).size == n // tm.D1 // 2
        t.set_filter(mover, 1, APB, 1_000)                                # ... and back
        assert t.slot(mover) == home
        m.set_audio_rate(mover, APB, 1_000, home)
        bank.reset(home)
        want_bank.reset(home)
        block(True)
        # it came back like a new receiver: not with the envelope it left behind in the slot, not with the histories it had
        on, target, fb, step, state = t.get_agc(mover)
        assert (on, fb, step) == (True, floor_bits, agc_np.design(*settings, 1_000)[2])
        assert not _same_bits(m.audio(mover), twin.audio(mover))
        assert not _same_bits(m.chan_iq(mover), twin.chan_iq(mover))
        for c in range(nrx):
            if c != mover and modes[c] != tm.FM:                          # the others: as if nothing had happened
                assert _same_bits(t.fetch(c, capi.WR_STAGE_AUDIO, n), twin.audio(c)), c
        block(True)
        block(True)
        assert int(want_bank.windows[home]) >= 2
    finally:
        dev.free(out)
        spec.destroy()
        bank.destroy()
        t.destroy()


# ---- 4: caller-designed taps ----------------------------------------------------------------------------------------------------

STAGES = {"channel": 0, "audio": 1, "second": 2}                          # WR_FILTER_CHANNEL, WR_FILTER_AUDIO, WR_FILTER_CHANNEL2


@pytest.mark.parametrize("nco", [capi.WR_NCO_EXACT, capi.WR_NCO_ROTATE], ids=["exact", "rotate"])
@pytest.mark.parametrize("length", [8, 64, 256])
@pytest.mark.parametrize("stage", ["channel", "audio", "second"])
def test_caller_designed_taps(dev, oracle, stage, length, nco):
    """wr_chan_set_taps_n with taps that no lowpass design would give: uniform(-1, 1) / length, asymmetric and of full size at
    every position (wr_lowpass_design's are a thousand times smaller at the ends than in the middle, so that an error at an end
    tap hides in the ROTATE tolerance).  One stage at a time on 70 receivers -- two receivers with a second tap set of their
    own -- over three blocks of 100, 20 and 60 frames at the demodulator.  The second is shorter than the audio filter's history
    at every length and than a 256-tap second stage's; a channel filter's history (up to 255 input frames) is shorter than
    any block that gives a receiver a frame, so for that stage the blocks differ in size only."""
    lib = dev.lib
    two = stage == "second"
    fs, d2, nrx = tm.FS, 5, 70
    d1, d1b = (40, 10) if two else (400, 1)
    r1 = fs // d1
    r_dem = r1 // d1b
    pb1, pb1b, pb2 = 128_000, r1 // 8, 160
    rng = np.random.default_rng(1000 * length + 10 * STAGES[stage] + nco)
    sets = [(rng.uniform(-1.0, 1.0, length) / length).astype(np.float32) for _ in range(2)]
    own = (5, 66)
    ifs = [(c - nrx // 2) * 25_000 + 321 for c in range(nrx)]
    modes = [tm.AM, tm.USB, tm.LSB]
    probe = [0, 1, 5, 33, 63, 64, 66, 69]
    decim = {"channel": d1, "audio": d2, "second": d1b}[stage]
    t = Tuner(dev, fs, nrx, 40_000, nco)
    try:
        for c, f in enumerate(ifs):
            ch = t.add_receiver(f, pb1, r1, modes[c % 3], pb2, r_dem // d2, stage2=(64, pb1b, r_dem) if two else None)
            taps = sets[c in own]
            if (stage, length, nco) == ("channel", 64, capi.WR_NCO_EXACT):
                capi.check(lib.wr_chan_set_taps(t.h, ch, STAGES[stage], capi.ptr(taps), decim))     # the 64-tap entry
            else:
                capi.check(lib.wr_chan_set_taps_n(t.h, ch, STAGES[stage], capi.ptr(taps), length, decim))
        # (blocks of several sizes: the oracle's filters keep their true histories, quirk Q7)
        rxs = {c: OracleChain(oracle, fs, ifs[c], 64, pb1, d1, modes[c % 3], 64, pb2, d2, stage2=(64, pb1b, d1b) if two else None,
                              taps={stage: sets[c in own]}, keep_history=True) for c in probe}
        gain = {s: max(1.0, float(np.abs(sets[s]).sum())) for s in (0, 1)}
        gain2 = max(1.0, float(np.abs(oracle.lowpass_design(pb2, r_dem)).sum()))
        pos, live = 0, 0.0
        iq = tm.signal(72_000, [ifs[c] for c in probe[::2]], seed=length)
        for n in (40_000, 8_000, 24_000):                                 # 100, 20 and 60 frames at the demodulator
            b = iq[2 * pos: 2 * (pos + n)]
            pos += n
            t.submit_host(b)
            for c in probe:
                wa, wc, _ = rxs[c].run(b)
                gc = t.fetch(c, capi.WR_STAGE_CHAN_IQ, 2 * n)
                ga = t.fetch(c, capi.WR_STAGE_AUDIO, n)
                assert gc.size == wc.size == 2 * (n // d1 // d1b) and ga.size == wa.size == n // d1 // d1b // d2, (n, c)
                if nco == capi.WR_NCO_EXACT:
                    assert np.array_equal(bits_f32(gc), bits_f32(wc)), (n, c)
                    assert np.array_equal(bits_f32(ga), bits_f32(wa)), (n, c)
                else:
                    g = gain[c in own]
                    assert float(np.abs(gc - wc).max()) <= IQ_ATOL, (n, c, float(np.abs(gc - wc).max()))
                    # |.| and the sums of Re and Im are 2-Lipschitz, then the linear audio filter (tunercases.py)
                    assert float(np.abs(ga - wa).max()) <= LINEAR_ATOL * (g if stage == "audio" else gain2), (n, c)
                live = max(live, float(np.abs(ga).max()))
        assert live > 1e-4                                                # a live channel, not zeros
        count = C.c_int()
        capi.check(lib.wr_chan_count(t.h, C.byref(count)))
        assert count.value == nrx
        t.remove_receiver(7)
        capi.check(lib.wr_chan_count(t.h, C.byref(count)))
        assert count.value == nrx - 1
    finally:
        t.destroy()
