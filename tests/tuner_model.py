"""A wr_tuner on the CPU, and the random scripts that the GPU tests of test_gpu_scripts.py play against it.

TunerModel is one wr_tuner put together from the yardsticks the suite already has and from nothing else: one
oracle.Receiver per receiver (mixer, channel filter, detector, audio filter), oracle.af_gain_squelch, agc_np.apply with the
state word carried from block to block, levels_np.levels, oracle.Spectrum and tones_np.Bank.  The order of a receiver's
audio is the header's: audio filter -> squelch -> AGC -> af_gain -> scale.  Setters are staged as the library stages them:
they act at the next submit (a seek uploads staged settings too), and the model keeps the copies "as of the last submit"
that `muted` of wr_tuner_chan_levels and the numbers of wr_chan_get_agc are documented to show.

One deliberate difference from a bare oracle.Receiver: the reference's LowPass loses its history when the block size
changes (quirk Q7, tests/test_gpu_blocks.py), the oracle copies that and the product deliberately does not.  Before a block of
another size the model therefore gives the oracle's two filters the buffer length of that size and puts their true last
L - 1 frames back (wr_oracle.fir_keep_history) -- with the oracle's own wro_fir_process, so that no filter arithmetic is restated here.

Behind the tuner sit the row banks, each as its numpy restatement (RowBanks): tones_np.Bank twice, and resamp_np.Bank,
dcs_np.Bank and voice_np.Bank with a second resamp_np.Bank behind it, all fed the rows of m.audio_rows().

make_script(seed) is a pure function: the operations, the block cuts and the configuration of one script.  script_stats()
walks a script without any signal processing and counts what test_tuner_model.py asserts on (the non-vacuity conditions).
"""
import os

import numpy as np

import agc_np
import dcs_np
import levels_np
import resamp_np
import tones_np
import voice_np
import wr_oracle as oracle

AM, FM, USB, LSB = range(4)
FS, CHAN_RATE, D1 = 2_000_000, 5_000, 400
CHAN_PASSBANDS = (128_000, 96_000, 200_000)          # LowPass bins 2, 1 and 3 of 64 taps at 2 MHz
AUDIO_PASSBAND = 160                                  # bin 1 at 5 kHz, as test_gpu_agc.py
BANK_WINDOWS = (16, 120)
CHAN_SPECTRUM_N = 64
AUDIO_SPECTRUM_N = 8                                  # the smallest size wr_spectrum_create_real takes
SQUELCH_DBFS = (-46.0, -44.0, -48.0)                  # test_gpu_chan_levels.test_the_gate's thresholds
GAINS_DB = (6.0, -3.5, -12.5, 0.0)
AGC_SETTINGS = ((-12.0, 20.0, 60.0), (-6.0, 5.0, 40.0), (-20.0, 60.0, 30.0), (-15.0, 40.0, 60.0))
# the row banks behind the tuner: a resampler audio_rate -> 3/4 of it, a voice bank whose output block goes on into a second,
# upsampling resampler (the chain the README recommends), and a DCS bank on a caller's step (wr_dcs_step refuses the scripts'
# audio rates): just over two frames per chip, an evaluation about every 16 audio frames
RESAMP_P, CHAIN_P, VOICE_T, VOICE_FILTERS = 32, 8, 64, 3
DCS_STEP, DCS_MAX_ERRORS = (1 << 28) - 54_321, 1
DCS_OCTAL = (0o023, 0o047, 0o754, 0o412, 0o131, 0o606)                 # six of DCS_CODES ...
DCS_OWN_WORDS = (0x2A5A5B, 0x000001)                                  # ... and two words that are nobody's code


def fuzz_seeds():
    return range(int(os.environ.get("WR_FUZZ_SEEDS", "8")))


class Rx:
    """one receiver: its oracle.Receiver, the staged settings, and the copies the last upload used"""

    def __init__(self, fs, if_hz, cpb, chan_rate, mode, apb, audio_rate, slot):
        self.fs, self.chan_rate, self.audio_rate, self.apb = fs, chan_rate, audio_rate, apb
        self.if_hz, self.cpb, self.mode, self.slot = if_hz, cpb, mode, slot
        self.rx = oracle.Receiver(fs, if_hz, cpb, chan_rate, mode, apb, audio_rate)
        self.gain_db, self.sq, self.agc = 0.0, None, None             # staged
        self.used_sq, self.used_agc = None, None                      # as of the last upload; used_agc: (target, floor, step)
        self.agc_state, self.agc_reset = 0, False
        self.was_fm = mode == FM
        self.last = None                                              # (audio, chan_iq, k1, k2) of the last submit

    @property
    def d2(self):
        return self.rx.d2

    def fresh(self, phase, prev):
        """empty filter histories; the NCO phase and the detector's previous frame as given"""
        self.rx = oracle.Receiver(self.fs, self.if_hz, self.cpb, self.chan_rate, self.mode, self.apb, self.audio_rate)
        self.rx.s.phase = phase
        self.rx.s.prev_i, self.rx.s.prev_q = prev
        self.was_fm = self.mode == FM

    def upload(self):
        """what wrc_group_upload does with the staged squelch and AGC"""
        self.used_sq = self.sq
        self.used_agc = agc_np.design(*self.agc, self.audio_rate) if self.agc else None
        if self.used_agc and self.agc_reset:
            self.agc_state = self.used_agc[1]
            self.agc_reset = False

    def gate(self):
        """(frames the squelch muted, ones and zeros per audio frame) of the last submit under the thresholds in use"""
        _, chan, _, k2 = self.last
        if self.used_sq is None or not k2:
            return 0, np.ones(k2, np.float32)
        g = oracle.af_gain_squelch(np.ones(k2, np.float32), chan, self.d2, 0.0, self.used_sq)
        return int(np.count_nonzero(g == 0.0)), g


class TunerModel:
    def __init__(self, fs=FS, scale=1.0):
        self.fs, self.scale = fs, np.float32(scale)
        self.rxs = {}                                                 # handle -> Rx
        self.submits = 0

    # ---- receivers coming and going ----------------------------------------------------------------------------------------
    def add(self, handle, slot, if_hz, cpb, chan_rate, mode, apb, audio_rate):
        assert handle not in self.rxs and slot not in [r.slot for r in self.rxs.values()]
        self.rxs[handle] = Rx(self.fs, if_hz, cpb, chan_rate, mode, apb, audio_rate, slot)

    def remove(self, handle):
        del self.rxs[handle]

    def set_audio_rate(self, handle, apb, audio_rate, slot):
        """wr_chan_set_filter on stage 1 with another out_rate: the receiver is seated anew -- empty histories, the phase and
        the detector's previous frame kept, the AGC from floor with a step for the new rate"""
        r = self.rxs[handle]
        r.apb, r.audio_rate, r.slot = apb, audio_rate, slot
        r.fresh(r.rx.s.phase, (r.rx.s.prev_i, r.rx.s.prev_q))
        r.agc_reset = True
        r.last = None

    # ---- setters: staged ---------------------------------------------------------------------------------------------------
    def set_if(self, handle, if_hz):
        r = self.rxs[handle]
        r.if_hz = if_hz
        r.rx.set_if(if_hz)

    def set_mode(self, handle, mode):
        r = self.rxs[handle]
        r.mode = mode
        r.rx.set_mode(mode)

    def set_chan_passband(self, handle, cpb):
        r = self.rxs[handle]
        r.cpb = cpb
        taps = oracle.lowpass_design(cpb, self.fs)
        for j, v in enumerate(taps):
            r.rx.s.chan_fir.coeff[j] = float(v)

    def set_af_gain(self, handle, db):
        self.rxs[handle].gain_db = float(db)

    def set_squelch(self, handle, dbfs):
        self.rxs[handle].sq = dbfs

    def set_agc(self, handle, settings):
        """settings: (target_dbfs, decay_db_per_s, max_gain_db) or None for off; coming on starts from floor, new settings
        keep the state"""
        r = self.rxs[handle]
        if settings is not None and r.agc is None:
            r.agc_reset = True
        r.agc = settings

    def reset_history(self, handle):
        r = self.rxs[handle]
        r.fresh(r.rx.s.phase, (r.rx.s.prev_i, r.rx.s.prev_q))         # quirk Q5: phase and prev_i/q are kept
        r.agc_reset = True

    def seek(self, frame):
        for r in self.rxs.values():
            r.upload()                                                # (a seek uploads staged settings too)
            r.fresh((oracle.phase_step(r.if_hz, self.fs) * frame) & 0x7FFFFFFF, (0.0, 0.0))
            if r.agc:
                r.agc_reset = True

    # ---- a block -----------------------------------------------------------------------------------------------------------
    def submit(self, iq):
        iq = np.ascontiguousarray(iq, np.float32)
        n = iq.size // 2
        for r in self.rxs.values():
            r.upload()
            r.was_fm = r.was_fm or r.mode == FM
            k1 = n // r.rx.d1
            oracle.fir_keep_history(r.rx.s.chan_fir, 2 * n)
            oracle.fir_keep_history(r.rx.s.audio_fir, k1)
            wa, wc, _ = r.rx.run(iq)
            if r.used_agc:
                target, floor_bits, step = r.used_agc
                v = oracle.af_gain_squelch(wa, wc, r.d2, 0.0, r.used_sq)
                gain = np.float32(10.0 ** (r.gain_db / 20.0))
                out, r.agc_state = agc_np.apply(v, target, floor_bits, step, r.agc_state, gain, self.scale) if v.size \
                    else (v, r.agc_state)
            else:
                out = oracle.af_gain_squelch(wa, wc, r.d2, r.gain_db, r.used_sq)
                if self.scale != np.float32(1.0):
                    out = (out * self.scale).astype(np.float32)
            r.last = (out, wc, k1, wa.size)
        self.submits += 1

    # ---- getters -----------------------------------------------------------------------------------------------------------
    def audio(self, handle):
        return self.rxs[handle].last[0]

    def chan_iq(self, handle):
        return self.rxs[handle].last[1]

    def phase(self, handle):
        return self.rxs[handle].rx.s.phase

    def levels(self, handle):
        """(mean, peak, muted) of the last submit's channel IQ"""
        r = self.rxs[handle]
        mean, peak = levels_np.levels(r.last[1])
        return mean, peak, r.gate()[0]

    def chan_spectrum(self, handle, first, n=CHAN_SPECTRUM_N):
        o = oracle.Spectrum(n)
        o.process(np.ascontiguousarray(self.rxs[handle].last[1][2 * first: 2 * (first + n)], np.float32))
        assert o.frames_done == 1
        return o.get()

    def audio_spectrum(self, handle, n=AUDIO_SPECTRUM_N):
        """the IQ sink fed (x, 0): the definition test_gpu_spectrum_real.py states"""
        x = self.rxs[handle].last[0][:n]
        iq = np.zeros(2 * n, np.float32)
        iq[0::2] = x
        o = oracle.Spectrum(n)
        o.process(iq)
        return o.get()

    def get_agc(self, handle):
        """(on, target, floor_bits, step, state) as the last upload used and the last submit left them"""
        r = self.rxs[handle]
        if not r.used_agc:
            return False, np.float32(0.0), 0, 0, 0
        return (True,) + tuple(r.used_agc) + (r.agc_state,)

    def agc_on(self):
        return sum(1 for r in self.rxs.values() if r.used_agc)

    def audio_rows(self, nrows):
        """the last submit's audio by slot; zeros where no receiver sits"""
        k2 = max([r.last[3] for r in self.rxs.values()] or [0])
        rows = np.zeros((nrows, k2), np.float32)
        for r in self.rxs.values():
            rows[r.slot] = r.last[0]
        return rows

    def fm_tolerance(self, handle):
        """4 * FM_ATOL * sum|audio taps| (test_gpu_fuzz.py), through the receiver's af_gain and the sink's scale"""
        r = self.rxs[handle]
        taps = oracle.lowpass_design(r.apb, r.chan_rate)
        return 4 * 2.4e-7 * max(1.0, float(np.abs(taps).sum())) * max(1.0, 10.0 ** (r.gain_db / 20.0)) * float(self.scale)

    def rotate_tolerance(self, handle):
        """2e-6 * sum|audio taps| (test_gpu_fuzz.py), through the receiver's af_gain and the sink's scale"""
        r = self.rxs[handle]
        taps = oracle.lowpass_design(r.apb, r.chan_rate)
        return 2e-6 * max(1.0, float(np.abs(taps).sum())) * max(1.0, 10.0 ** (r.gain_db / 20.0)) * float(self.scale)


# ---- the signal ---------------------------------------------------------------------------------------------------------------

def signal(nframes, carriers, seed, fs=FS):
    """noise in every channel and a carrier keyed at 150 Hz on each of `carriers` (test_gpu_agc._block's signal), as one
    stream of nframes frames"""
    tt = np.arange(nframes) / fs
    iq = (0.002 * np.random.default_rng(77_000 + seed).standard_normal(2 * nframes)).astype(np.float32)
    env = 0.02 * (1.0 + np.sign(np.sin(2 * np.pi * 150.0 * tt))) * 0.5
    for f in carriers:
        ph = 2 * np.pi * ((f * tt) % 1.0)
        iq[0::2] += (env * np.cos(ph)).astype(np.float32)
        iq[1::2] += (env * np.sin(ph)).astype(np.float32)
    return iq


# ---- scripts ------------------------------------------------------------------------------------------------------------------

SUBMIT_KINDS = ("dev", "other", "ragged", "short", "host")
SETTER_KINDS = ("set_if", "set_mode", "set_filter", "af_gain", "squelch_on", "squelch_off", "squelch_thr", "agc_on", "agc_off",
                "agc_new", "reset_history", "seek", "remove", "add")
GETTER_KINDS = ("fetch_audio", "fetch_chan", "fetch_all", "levels", "spectra", "tones", "tones_again", "audio_spectrum",
                "get_agc", "state", "flush", "drain")
# the row banks behind the tone bank: they enter a script in a pass of their own (_with_banks), so GETTER_KINDS, which the
# first pass draws from, stays what it was
PUSH_KINDS = ("resamp", "dcs", "voice")
BANK_KINDS = PUSH_KINDS + tuple(k + "_again" for k in PUSH_KINDS) + ("voice_ctl",)
ALL_KINDS = tuple("submit_" + k for k in SUBMIT_KINDS) + SETTER_KINDS + GETTER_KINDS + BANK_KINDS
# frames of history a bank keeps per row: a push of fewer frames takes the history writers' "nframes < H" branch
BANK_HISTORY = {"resamp": RESAMP_P - 1, "voice": VOICE_T - 1, "chain": CHAIN_P - 1}
# getters whose answer is about "the last submit": with wr_tuner_set_blocks_per_launch that is the whole group of held blocks,
# so a script asks them only where at most one block can be held (a flush goes in front of that block otherwise)
_LAST_SUBMIT_GETTERS = ("fetch_audio", "fetch_chan", "fetch_all", "levels", "spectra", "tones", "audio_spectrum")


def kind_of(op):
    return "submit_" + op[1] if op[0] == "submit" else op[0]


def _ifs(nrx):
    spacing = 25_000 if nrx <= 70 else 15_000
    return [(c - nrx // 2) * spacing + 321 for c in range(nrx)]


def make_script(seed, banks=True):
    """The script of a seed: a dict with the tuner's shape ("nrx", "max_channels", "d2", "audio_rate", "scale", "usual",
    "max_block", "hold", "ifs", "carriers", "total"), the operations "ops" and the block cuts "cuts" [(first frame, frames)].

    Operations, as tuples (c is a receiver's handle, the index wr_chan_add returns: the lowest free one):
      ("submit", kind, frames)      kind: dev / other / ragged / short (device memory, following on) or host
      ("set_if", c, hz) ("set_mode", c, mode) ("set_filter", c, passband) ("af_gain", c, dB)
      ("squelch_on", c, dBFS) ("squelch_thr", c, dBFS) ("squelch_off", c)
      ("agc_on", c, settings) ("agc_new", c, settings) ("agc_off", c)
      ("reset_history", c) ("seek", frame) ("remove", c) ("add", c, slot, hz, mode) ("bank_reset", slot or -1)
      ("fetch_audio", c) ("fetch_chan", c) ("fetch_all",) ("levels",) ("spectra", first_frame) ("tones", bank)
      ("tones_again", bank) ("audio_spectrum",) ("get_agc", c) ("state", c) ("flush",) ("drain",)
    and, with `banks` (_with_banks: a second pass with a generator of its own; banks=False is the first pass alone):
      ("resamp",) ("dcs",) ("voice",)   the last submit into the resampler, the DCS bank, the voice bank and on into a second resampler
      ("resamp_again",) ("dcs_again",) ("voice_again",)   the same submit pushed twice: refused, nothing counted
      ("voice_ctl", slot, word)         a row's control word: the filter index and the mute bit, from the next push on
    Guarantees: only receivers with c % 4 == 1 are ever FM; an add, a reset_history and a seek are followed by the bank resets
    the header asks of callers; squelch and AGC go to at most 8 receivers each, none of them ever FM, and the squelched ones
    sit on keyed carriers and are never retuned."""
    rng = np.random.default_rng(31_000 + seed)
    nrx = (5, 64, 70, 128)[seed % 4]
    d2 = (5, 5, 2, 5, 5, 1, 5, 5)[seed % 8]
    q = D1 * d2
    # the usual block: 13 to 20 audio frames at D2 = 5; at least 64 channel-rate frames at every D2, so that it streams
    frames = int(rng.integers(13, 21)) if d2 == 5 else -(-64 // d2) + int(rng.integers(1, 8))
    usual = q * frames
    hold = int(rng.integers(2, 5))
    ifs = _ifs(nrx)
    plain = [c for c in range(nrx) if c % 4 != 1]                          # never FM
    pick = [int(c) for c in rng.permutation(plain)]
    n_sq, n_agc = (2, 2) if nrx == 5 else (4, 5)
    sq_set = sorted(pick[:n_sq])
    agc_set = sorted(pick[n_sq - 1: n_sq - 1 + n_agc])                     # one receiver has both
    carriers = [ifs[c] for c in sq_set]

    ops, cuts = [], []
    st = {"pos": 0, "k1": 0, "k2": 0, "group": 0, "open": False, "pushed": set(), "submitted": False}
    live = {c: c for c in range(nrx)}                                     # handle -> slot
    modes = {c: c % 4 for c in range(nrx)}
    cur_if = dict(enumerate(ifs))
    sq_on, agc_on, gone = set(), set(), []

    def emit(op):
        # st["group"]: how many blocks the launch of the last submit may cover when blocks are held; st["open"]: the next
        # submit may still join it (nothing has touched the tuner since)
        if op[0] in _LAST_SUBMIT_GETTERS and st["group"] >= 2:
            at = max(i for i, o in enumerate(ops) if o[0] == "submit")
            ops.insert(at, ("flush",))
            st["group"] = 1
        st["open"] = False
        ops.append(op)

    def submit(kind):
        if kind == "dev":
            n = usual
        elif kind == "other":
            n = q * (frames + int(rng.integers(2, 6)))
        elif kind == "ragged":
            n = usual + int(rng.integers(1, q))
        elif kind == "short":                                             # fewer channel-rate frames than the audio filter's history
            n = q * int(rng.integers(2, max(3, 62 // d2 + 1)))
        else:
            n = usual
        st["group"] = st["group"] + 1 if st["open"] and not agc_on else 1
        ops.append(("submit", kind, n))
        st["open"] = True
        cuts.append((st["pos"], n))
        st["pos"] += n
        st["k1"], st["k2"] = n // D1, n // D1 // d2
        st["pushed"] = set()
        st["submitted"] = True

    def some(cands):
        cands = [c for c in cands if c in live]
        return int(rng.choice(cands)) if cands else None

    def setter(kind):
        want = None
        if isinstance(kind, tuple):                                       # (kind, the receiver it goes to)
            kind, want = kind
        if kind == "set_if":
            c = some([c for c in live if c not in sq_set])
            cur_if[c] = int(rng.integers(-FS // 2 + 1, FS // 2))
            emit(("set_if", c, cur_if[c]))
        elif kind == "set_mode":
            c = some(list(live))
            modes[c] = int(rng.integers(0, 4)) if c % 4 == 1 else int(rng.choice([AM, USB, LSB]))
            emit(("set_mode", c, modes[c]))
        elif kind == "set_filter":
            emit(("set_filter", some(list(live)), int(rng.choice(CHAN_PASSBANDS))))
        elif kind == "af_gain":
            emit(("af_gain", want if want is not None else some(list(live)),
                  float(rng.choice(GAINS_DB[:3] if want is not None else GAINS_DB))))
        elif kind in ("squelch_on", "squelch_thr"):
            c = want if want is not None else some([c for c in sq_set if (c in sq_on) == (kind == "squelch_thr")])
            if c is not None:
                sq_on.add(c)
                emit((kind, c, float(rng.choice(SQUELCH_DBFS))))
        elif kind == "squelch_off":
            c = some(list(sq_on))
            if c is not None:
                sq_on.discard(c)
                emit(("squelch_off", c))
        elif kind in ("agc_on", "agc_new"):
            c = want if want is not None else some([c for c in agc_set if (c in agc_on) == (kind == "agc_new")])
            if c is not None:
                agc_on.add(c)
                emit((kind, c, AGC_SETTINGS[int(rng.integers(len(AGC_SETTINGS)))]))
        elif kind == "agc_off":
            c = want = some(list(agc_on))
            if c is not None:
                agc_on.discard(c)
                emit(("agc_off", c))
        elif kind == "reset_history":
            c = some(list(live))
            emit(("reset_history", c))
            emit(("bank_reset", live[c]))
        elif kind == "seek":
            emit(("seek", st["pos"]))
            emit(("bank_reset", -1))
        elif kind == "remove":
            # the receiver that leaves has its AGC on and an af_gain, in every other seed a squelch as well: what it leaves
            # behind in the slot (envelope, threshold, gain, histories, bank row) must not reach the receiver seated there next
            c = want
            assert c in agc_on and c in live
            sq_on.discard(c)
            agc_on.discard(c)
            gone.append((c, live.pop(c)))
            emit(("remove", c))
        elif kind == "add" and gone:
            gone.sort()
            c, _ = gone.pop(0)                                            # wr_chan_add: the lowest free handle ...
            slot = min(set(range(nrx + 3)) - set(live.values()))          # ... chan_seat: the lowest free slot
            live[c] = slot
            modes[c] = c % 4 if c % 4 != 1 else int(rng.choice([AM, FM]))
            emit(("add", c, slot, cur_if[c], modes[c]))
            emit(("bank_reset", slot))
        if st["submitted"] and kind in ("squelch_thr", "squelch_off", "agc_new", "agc_off") and want is None or kind == "agc_off":
            # a setting changed and asked about before the next submit: the answer is still the last submit's
            emit(("levels",) if kind.startswith("squelch") else ("get_agc", c if c is not None else some(agc_set)))

    def getter(kind):
        if kind in ("fetch_audio", "fetch_chan", "state"):
            emit((kind, some(list(live))))
        elif kind == "get_agc":
            emit((kind, some(agc_set)))
        elif kind == "spectra":
            if st["k1"] >= CHAN_SPECTRUM_N:
                emit((kind, int(rng.integers(0, st["k1"] - CHAN_SPECTRUM_N + 1))))
        elif kind == "audio_spectrum":
            if st["k2"] >= AUDIO_SPECTRUM_N:
                emit((kind,))
        elif kind == "tones":
            for b in range(len(BANK_WINDOWS)):
                if b not in st["pushed"]:
                    st["pushed"].add(b)
                    emit((kind, b))
        elif kind == "tones_again":
            if st["pushed"]:
                emit((kind, int(rng.choice(sorted(st["pushed"])))))
        else:
            emit((kind,))

    run_at = int(rng.integers(1, 3))                                      # rounds run_at .. run_at + 3: four device blocks in a row
    quiet = set(range(run_at + 1, run_at + 4))                            # ... with nothing in front of the last three
    silent = set(range(run_at, run_at + 3))                               # ... and nothing behind the first three
    agc_from = run_at + 4
    agc_till = agc_from + 2 + int(rng.integers(0, 2))
    rounds = agc_till + 4
    free = [r for r in range(rounds) if r not in quiet and r != run_at]
    late = [r for r in free if r > run_at + 3]

    def turn(names, every, base):
        """the kinds whose turn it is in this seed: each comes up in one seed out of `every`"""
        return [k for i, k in enumerate(names) if (i + base + seed) % every == 0]

    kinds = {r: "dev" for r in range(rounds)}
    for k, r in zip(turn(("other", "ragged", "short", "host"), 2, 0), rng.permutation([r for r in free if r > 0])):
        kinds[int(r)] = k
    for r in free:
        if kinds[r] == "dev" and rng.random() < 0.2:
            kinds[r] = str(rng.choice(SUBMIT_KINDS))
    before = {r: [] for r in range(rounds)}
    for c in sq_set:
        before[0].append("squelch_on")
    for c in agc_set:
        before[agc_from].append("agc_on")
        before[agc_till].append("agc_off")
    # one receiver leaves while its AGC is on and has run, and comes back into the slot it left; a block or more later the
    # newcomer gets an AGC, an af_gain and (where it sits on a carrier) a squelch of its own
    both = [c for c in agc_set if c in sq_set]
    leaver = both[0] if seed % 2 == 0 else [c for c in agc_set if c not in sq_set][seed // 2 % (len(agc_set) - 1)]
    before[agc_from].append(("af_gain", leaver))
    r_rm = int(rng.integers(agc_from + 1, agc_till + 1))
    r_add = r_rm + int(rng.integers(0, 2))
    before[r_rm].append(("remove", leaver))
    before[r_add].append("add")
    r_on = max(r_add + 1, agc_till + 1)
    before[r_on].append(("agc_on", leaver))
    before[r_on + int(rng.integers(0, 2))].append(("af_gain", leaver))
    if leaver in sq_set:
        before[r_on + int(rng.integers(0, 2))].append(("squelch_on", leaver))
    for k in turn(("set_if", "set_mode", "set_filter", "af_gain", "squelch_thr", "reset_history", "squelch_off", "seek"), 2, 0):
        before[int(rng.integers(1, run_at + 1)) if k == "seek" else int(rng.choice(late if k == "squelch_off" else free))].append(k)
    if seed % 2:
        before[int(rng.integers(agc_from + 1, agc_till + 1))].append("agc_new")
    for _ in range(2):
        before[int(rng.choice(free))].append(str(rng.choice(["set_if", "set_mode", "set_filter", "af_gain", "squelch_thr"])))
    odds = {"tones": 1.0, "levels": 0.25, "spectra": 0.2, "fetch_audio": 0.3, "fetch_chan": 0.2, "fetch_all": 0.2,
            "audio_spectrum": 0.15, "get_agc": 0.2, "state": 0.15, "flush": 0.08, "drain": 0.15, "tones_again": 0.1}
    after = {r: [] if r in silent else [k for k in GETTER_KINDS if rng.random() < odds[k]] for r in range(rounds)}
    full = [r for r in range(rounds) if r not in silent and kinds[r] != "short"]
    for k in turn(GETTER_KINDS, 3, 1):
        if not any(k in after[r] for r in full):
            after[int(rng.choice(full))].append(k)
    for r in range(rounds):
        for k in sorted(before[r], key=lambda k: (k == "add", k in ("agc_off", "squelch_off")) if isinstance(k, str) else
                        (k[0] != "remove", False)):
            setter(k)
        if r in quiet:
            assert ops[-1][0] == "submit"
        submit(kinds[r])
        order = [k for k in after[r] if k != "tones_again"]
        order = [order[i] for i in rng.permutation(len(order))] if order else []
        if "tones_again" in after[r]:
            order = ["tones"] + [k for k in order if k != "tones"] + ["tones_again"]
        for k in order:
            getter(k)
    while gone:
        setter("add")
        submit("dev")
        getter("tones")
        getter("fetch_all")
    # until every bank has latched a window on a row that stays bit for bit: more blocks, each pushed
    while min(script_stats({"ops": ops, "nrx": nrx, "d2": d2})["latched"]) < 1:
        submit("dev")
        getter("tones")
    emit(("flush",))
    emit(("drain",))
    script = {"seed": seed, "nrx": nrx, "max_channels": nrx + 3, "d2": d2, "audio_rate": CHAN_RATE // d2, "frames": frames,
              "scale": (1.0, 32768.0)[seed % 2], "usual": usual, "max_block": usual * hold + q, "hold": hold, "ifs": ifs,
              "carriers": carriers, "sq_set": sq_set, "agc_set": agc_set, "ops": ops, "cuts": cuts, "total": st["pos"]}
    if banks:
        script["ops"] = _with_banks(script)
    return script


def _with_banks(script):
    """The operations of `script` with the three row banks played in: with BANK_KINDS filtered out again, the list is the one
    that came in.  The pushes are "last submit" getters and stand only where the script pushes the tone banks after a submit
    -- there the flush in front of a held group is in place, and the run of device blocks with nothing between them stays
    as it is -- in a random order among themselves and among the tone pushes, so each is sometimes the first operation after
    a submit; now and then a bank skips a submit.  A voice_ctl stands where a setter may stand: in front of a submit that
    already has something in front of it, or between a submit and its voice push.  In every script one row of a receiver
    that is never FM and never leaves is muted, pushed, and un-muted again."""
    seed, base = script["seed"], script["ops"]
    rng = np.random.default_rng(41_000 + seed)
    live = {c: c for c in range(script["nrx"])}                           # handle -> slot
    stays = [c for c in live if c % 4 != 1 and c not in {op[1] for op in base if op[0] == "remove"}]
    mute_row = int(rng.choice(stays))
    mute_plan = ["mute", "unmute"]
    pushed_muted = False

    def ctl(row=None, mute=None):
        if row is None:
            row = int(rng.choice(sorted(live.values())))
        if mute is None:
            mute = bool(rng.random() < 0.3)
            if row == mute_row and mute_plan:                             # (the planned row keeps the bit the plan gave it)
                mute = mute_plan[0] == "unmute"
        return ("voice_ctl", row, int(rng.integers(0, VOICE_FILTERS)) | (voice_np.MUTE if mute else 0))

    out, i, spans = [], 0, 0
    total = sum(1 for j, op in enumerate(base) if op[0] == "tones" and base[j - 1][0] != "tones")
    assert total >= 2, seed
    while i < len(base):
        op = base[i]
        if op[0] == "remove":
            del live[op[1]]
        elif op[0] == "add":
            live[op[1]] = op[2]
        if op[0] == "submit" and out and out[-1][0] != "submit" and rng.random() < 0.25:
            out.append(ctl())
        if op[0] != "tones":
            out.append(op)
            i += 1
            continue
        seq = []
        while i < len(base) and base[i][0] == "tones":
            seq.append(base[i])
            i += 1
        last = spans == total - 1
        new = [k for k in PUSH_KINDS if spans == 0 or rng.random() < 0.85 or (last and k == "voice")]
        for j in rng.permutation(len(new)):
            seq.insert(int(rng.integers(0, len(seq) + 1)), (new[int(j)],))
        if "voice" in new:
            planned = None
            if mute_plan and (mute_plan[0] == "mute" or pushed_muted) and (spans == 0 or last or rng.random() < 0.5):
                planned = ctl(mute_row, mute_plan[0] == "mute")
                mute_plan.pop(0)
            elif rng.random() < 0.3:
                planned = ctl()
            if planned:
                seq.insert(int(rng.integers(0, seq.index(("voice",)) + 1)), planned)
            pushed_muted = pushed_muted or mute_plan == ["unmute"]
        for n, k in enumerate(PUSH_KINDS):
            if k in new and (rng.random() < 0.15 or (spans == 0 and n == seed % 3)):
                seq.insert(int(rng.integers(seq.index((k,)) + 1, len(seq) + 1)), (k + "_again",))
        out += seq
        spans += 1
    assert not mute_plan, (seed, mute_plan)
    assert [op for op in out if op[0] not in BANK_KINDS] == base
    return out


def script_stats(script):
    """What a script holds, from its operations alone: {"kinds": count per operation kind, "run": the longest run of usual
    device blocks with nothing between them and no AGC on, "agc_on" / "agc_off": submits with / without an AGC in use,
    "reseated": adds into a slot that a removed receiver left, "reseated_agc" ("reseated_squelch"): submits in which a receiver
    seated in such a slot has an AGC (a squelch) on, where the receiver that left had run a block with its AGC (squelch) on,
    "asked": getters of a submit's levels or AGC numbers that follow a setter with no submit in between, "latched": per bank
    the most windows a row completed whose receiver is never FM, "first": per push kind of the row banks how often it is the
    first operation after a submit, "short": per bank ("chain": the second resampler behind the voice bank) the pushes of
    fewer frames than a row's history, "zero_out": pushes of the resampler that yield no frame, "ctl_pushed": voice pushes
    behind a voice_ctl, "ctl_late": those whose voice_ctl stands between the submit and its push, "unmuted": live rows
    pushed un-muted after they were pushed muted}"""
    ops, nrx, d2 = script["ops"], script["nrx"], script["d2"]
    kinds = {k: 0 for k in ALL_KINDS}
    agc, run, best, on, off, reseated = set(), 0, 0, 0, 0, 0
    sq, ran_agc, ran_sq, left_agc, left_sq, heirs = set(), set(), set(), set(), set(), {}
    re_agc, re_sq, asked, staged, submitted = 0, 0, 0, False, False
    vacated, slot_of = set(), {c: c for c in range(nrx)}
    fill = [dict() for _ in BANK_WINDOWS]                                 # bank -> slot -> frames since the row's reset
    latched = [0 for _ in BANK_WINDOWS]
    k2 = 0
    first = {k: 0 for k in PUSH_KINDS}
    short = {k: 0 for k in BANK_HISTORY}
    nmod, zero_out, ctl_since, ctl_pushed, ctl_late, was_muted, unmuted, words = 0, 0, None, 0, 0, set(), 0, {}
    for at, op in enumerate(ops):
        if op[0] != "bank_reset":
            kinds[kind_of(op)] += 1
        if op[0] in PUSH_KINDS:
            first[op[0]] += at > 0 and ops[at - 1][0] == "submit"
        if op[0] == "resamp":
            short["resamp"] += k2 < BANK_HISTORY["resamp"]
            zero_out += resamp_np.ceil_div((nmod + k2) * 3, 4) == resamp_np.ceil_div(nmod * 3, 4)
            nmod = (nmod + k2) % 4
        elif op[0] == "voice":
            short["voice"] += k2 < BANK_HISTORY["voice"]
            short["chain"] += k2 < BANK_HISTORY["chain"]
            ctl_pushed += ctl_since is not None
            ctl_late += ctl_since == "late"
            ctl_since = None
            for s in slot_of.values():
                if words.get(s, 0) & voice_np.MUTE:
                    was_muted.add(s)
                elif s in was_muted:
                    was_muted.discard(s)
                    unmuted += 1
        elif op[0] == "voice_ctl":
            words[op[1]] = op[2]
            ctl_since = "late" if submitted else "early"                  # (late: behind the submit whose push comes next)
        if op[0] == "bank_reset" and op[1] < 0:
            nmod = 0
        if op[0] == "submit":
            run = run + 1 if op[1] == "dev" and not agc else 0
            best = max(best, run)
            on, off = on + bool(agc), off + (not agc)
            k2 = op[2] // D1 // d2
            ran_agc |= agc
            ran_sq |= sq
            re_agc += any(c in agc and "agc" in what for c, what in heirs.items())
            re_sq += any(c in sq and "squelch" in what for c, what in heirs.items())
            staged, submitted = False, True
            if ctl_since:
                ctl_since = "early"                                       # (a word set before the submit that is pushed)
            continue
        run = 0
        if op[0] in SETTER_KINDS:
            staged = True
        if op[0] in ("levels", "get_agc") and staged and submitted:
            asked += 1
        if op[0] in ("squelch_on", "squelch_thr"):
            sq.add(op[1])
        elif op[0] == "squelch_off":
            sq.discard(op[1])
        if op[0] in ("agc_on", "agc_new"):
            agc.add(op[1])
        elif op[0] == "agc_off":
            agc.discard(op[1])
        elif op[0] == "remove":
            slot = slot_of.pop(op[1])
            vacated.add(slot)
            if op[1] in ran_agc and op[1] in agc:
                left_agc.add(slot)
            if op[1] in ran_sq and op[1] in sq:
                left_sq.add(slot)
            for group in (agc, sq, ran_agc, ran_sq):
                group.discard(op[1])
            heirs.pop(op[1], None)
        elif op[0] == "add":
            reseated += op[2] in vacated
            heirs[op[1]] = ["agc"] * (op[2] in left_agc) + ["squelch"] * (op[2] in left_sq)
            slot_of[op[1]] = op[2]
        elif op[0] == "bank_reset":
            for f in fill:
                if op[1] < 0:
                    f.clear()
                else:
                    f.pop(op[1], None)
        elif op[0] == "tones":
            for c, s in slot_of.items():
                if c % 4 != 1:
                    fill[op[1]][s] = fill[op[1]].get(s, 0) + k2
                    latched[op[1]] = max(latched[op[1]], fill[op[1]][s] // BANK_WINDOWS[op[1]])
    return {"kinds": kinds, "run": best, "agc_on": on, "agc_off": off, "reseated": reseated, "reseated_agc": re_agc,
            "reseated_squelch": re_sq, "asked": asked, "latched": latched, "first": first, "short": short,
            "zero_out": zero_out, "ctl_pushed": ctl_pushed, "ctl_late": ctl_late, "unmuted": unmuted}


# ---- a script played on the model ---------------------------------------------------------------------------------------------

def bank_steps(audio_rate):
    """the 50 CTCSS steps at this audio rate"""
    from webradio_amd import CTCSS_HZ
    return [tones_np.step_of(hz, audio_rate) for hz in CTCSS_HZ]


def slot_rows(max_channels):
    return (max_channels + 63) // 64 * 64


def audio_pos(script, pos):
    """the stream's position in audio frames at input frame `pos`: where wr_dcs_seek puts a bank that joins there"""
    return pos // (D1 * script["d2"])


def bank_shapes(script):
    """what a script's row banks are made with: {"resamp": (L, M, taps[L][P]) with wr_resamp_design's taps for audio_rate ->
    3/4 of it, "chain": (L, M, taps) of the upsampler behind the voice bank, 4/3 with a caller's rough taps of full size,
    "voice": taps[3][T], two seeded random filters and the unit impulse at T / 2 - 1, "words": the DCS bank's eight}"""
    from webradio_amd import DCS_CODES
    from webradio_amd.device import resamp_design
    rate = script["audio_rate"]
    taps, L, M = resamp_design(rate, rate * 3 // 4, RESAMP_P)
    assert (L, M) == (3, 4) and not [c for c in DCS_OCTAL if c not in DCS_CODES]
    rng = np.random.default_rng(43_000 + script["seed"])
    chain = rng.uniform(-16.0, 16.0, (4, CHAIN_P)).astype(np.float32)
    voice = rng.uniform(-1.0, 1.0, (VOICE_FILTERS, VOICE_T)).astype(np.float32)
    voice[2] = 0.0
    voice[2, VOICE_T // 2 - 1] = 1.0
    return {"resamp": (L, M, taps), "chain": (4, 3, chain), "voice": voice,
            "words": [dcs_np.word(c) for c in DCS_OCTAL] + list(DCS_OWN_WORDS)}


class RowBanks:
    """the restatements of a script's three row banks and of the resampler behind the voice bank, all of slot_rows rows and
    fed rows[nrows][frames]: the model's rows (ModelPlay) or the library's own (test_gpu_scripts.GpuPlay)"""

    def __init__(self, script):
        shapes, rows = bank_shapes(script), slot_rows(script["max_channels"])
        self.script = script
        self.resamp = resamp_np.Bank(rows, *shapes["resamp"])
        self.chain = resamp_np.Bank(rows, *shapes["chain"])
        self.voice = voice_np.Bank(rows, shapes["voice"])
        self.voice.set_rows(0, np.arange(rows) % VOICE_FILTERS)
        self.dcs = dcs_np.Bank(rows, shapes["words"], DCS_STEP, DCS_MAX_ERRORS)
        self.zero_out = 0                                                 # pushes of a resampler that yielded no frame

    def reset(self, row, pos):
        """what a script's bank_reset does to these banks, at input frame `pos` of the stream"""
        self.resamp.reset(row)
        self.chain.reset(row)
        self.voice.reset(row)
        if row >= 0 or self.script["seed"] % 2 == 0:
            self.dcs.reset(row)
        else:
            self.dcs.seek(audio_pos(self.script, pos))

    def push_resamp(self, rows):
        y = self.resamp.push(rows)
        self.zero_out += y.shape[1] == 0
        return y

    def push_dcs(self, rows):
        self.dcs.push(rows)
        return self.read_dcs()

    def read_dcs(self):
        return tuple(a.copy() for a in self.dcs.read())

    def push_voice(self, rows):
        """(the voice bank's frames, the frames of the resampler they go on into)"""
        y = self.voice.push(rows)
        z = self.chain.push(y)
        self.zero_out += z.shape[1] == 0
        return y, z

    def counts(self, kind):
        """the frame counts the bank's *_info call shows"""
        if kind == "resamp":
            return self.resamp.frames_in, self.resamp.frames_out
        if kind == "dcs":
            return (self.dcs.N,)
        return self.voice.frames, self.chain.frames_in, self.chain.frames_out


def dcs_by_slot(read, slots):
    agree, run, hits, evals = read
    return {s: (agree[s].copy(), run[s].copy(), hits[s].copy(), int(evals[s])) for s in slots}


class ModelPlay:
    """plays a script's operations on a TunerModel, two tones_np.Banks and the RowBanks; do(op) returns what the operation hands back:
      fetch_audio / fetch_chan   the array
      fetch_all                  {slot: audio}
      drain                      [(submit number, {slot: audio}, {slot: (bit for bit under WR_NCO_EXACT?, else the FM tolerance
                                 or None, the ROTATE tolerance or None)})]: a receiver's standing when the block was made
      levels                     ({handle: (mean, peak, muted)}, frames, audio_frames)
      spectra, audio_spectrum    {handle: dB row}
      tones, tones_again         the bank as {slot: (iq, energy, windows, fill)} for the live receivers
      resamp                     (output frames, {slot: frames}) for the live receivers
      dcs                        {slot: (agree, run, hits, evals)}
      voice                      ({slot: voice frames}, output frames of the second resampler, {slot: its frames})
      resamp_again, voice_again  the banks' frame counts as wr_resamp_info and wr_voice_info show them
      dcs_again                  ((frames,), the bank as for dcs)
      get_agc                    (on, target, floor_bits, step, state)
      state                      the NCO phase"""

    def __init__(self, script, iq):
        self.s, self.iq = script, iq
        self.m = TunerModel(FS, script["scale"])
        for c, f in enumerate(script["ifs"]):
            self.m.add(c, c, f, CHAN_PASSBANDS[0], CHAN_RATE, c % 4, AUDIO_PASSBAND, script["audio_rate"])
        rows = slot_rows(script["max_channels"])
        self.banks = [tones_np.Bank(rows, bank_steps(script["audio_rate"]), w) for w in BANK_WINDOWS]
        self.rb = RowBanks(script)
        self.rows = rows
        self.pos = 0
        self.ring = []

    def bank(self, b):
        iq, energy, windows, fill = self.banks[b].read()
        return {r.slot: (iq[r.slot].copy(), int(energy[r.slot]), int(windows[r.slot]), int(fill[r.slot]))
                for r in self.m.rxs.values()}

    def slots(self):
        return [r.slot for r in self.m.rxs.values()]

    def do(self, op):
        m, k = self.m, op[0]
        if k == "submit":
            m.submit(self.iq[2 * self.pos: 2 * (self.pos + op[2])])
            self.pos += op[2]
            self.ring.append((m.submits - 1, {r.slot: r.last[0] for r in m.rxs.values()},
                              {r.slot: (not r.was_fm, None if r.used_agc else m.fm_tolerance(c),
                                        m.rotate_tolerance(c) if c % 4 != 1 and not r.used_agc and r.used_sq is None else None)
                               for c, r in m.rxs.items()}))
        elif k == "set_if":
            m.set_if(op[1], op[2])
        elif k == "set_mode":
            m.set_mode(op[1], op[2])
        elif k == "set_filter":
            m.set_chan_passband(op[1], op[2])
        elif k == "af_gain":
            m.set_af_gain(op[1], op[2])
        elif k in ("squelch_on", "squelch_thr"):
            m.set_squelch(op[1], op[2])
        elif k == "squelch_off":
            m.set_squelch(op[1], None)
        elif k in ("agc_on", "agc_new"):
            m.set_agc(op[1], op[2])
        elif k == "agc_off":
            m.set_agc(op[1], None)
        elif k == "reset_history":
            m.reset_history(op[1])
        elif k == "seek":
            m.seek(op[1])
        elif k == "remove":
            m.remove(op[1])
        elif k == "add":
            m.add(op[1], op[2], op[3], CHAN_PASSBANDS[0], CHAN_RATE, op[4], AUDIO_PASSBAND, self.s["audio_rate"])
        elif k == "bank_reset":
            for b in self.banks:
                b.reset(op[1])
            self.rb.reset(op[1], self.pos)
        elif k == "voice_ctl":
            self.rb.voice.set_rows(op[1], [op[2]])
        elif k == "resamp":
            y = self.rb.push_resamp(m.audio_rows(self.rows))
            return y.shape[1], {s: y[s] for s in self.slots()}
        elif k == "dcs":
            return dcs_by_slot(self.rb.push_dcs(m.audio_rows(self.rows)), self.slots())
        elif k == "voice":
            y, z = self.rb.push_voice(m.audio_rows(self.rows))
            return {s: y[s] for s in self.slots()}, z.shape[1], {s: z[s] for s in self.slots()}
        elif k == "dcs_again":
            return self.rb.counts("dcs"), dcs_by_slot(self.rb.read_dcs(), self.slots())
        elif k in ("resamp_again", "voice_again"):
            return self.rb.counts(k[:-6])
        elif k == "fetch_audio":
            return m.audio(op[1])
        elif k == "fetch_chan":
            return m.chan_iq(op[1])
        elif k == "fetch_all":
            return {r.slot: r.last[0] for r in m.rxs.values()}
        elif k == "levels":
            any_rx = next(iter(m.rxs.values()))
            return {c: m.levels(c) for c in m.rxs}, any_rx.last[2], any_rx.last[3]
        elif k == "spectra":
            return {c: m.chan_spectrum(c, op[1]) for c in m.rxs}
        elif k == "audio_spectrum":
            return {c: m.audio_spectrum(c) for c in m.rxs}
        elif k == "tones":
            self.banks[op[1]].push(m.audio_rows(self.rows))
            return self.bank(op[1])
        elif k == "tones_again":
            return self.bank(op[1])
        elif k == "get_agc":
            return m.get_agc(op[1])
        elif k == "state":
            return m.phase(op[1])
        elif k == "drain":
            out, self.ring = self.ring, []
            return out
        return None
