"""-m gpu: what wr_chan_fetch and the five whole-tuner readers (wr_tuner_audio_dev, wr_tuner_chan_spectra,
wr_tuner_chan_levels, wr_tuner_tones_push, wr_tuner_fetch_audio_all) answer when they refuse, and what a refusal leaves
behind.  A characterisation: every expected value below is what the library did before its tuner source was split into
wr_tuner.hip, wr_tuner_submit.hip and wr_tuner_read.hip, not what the split code does.

One tuner of three receivers in one lane group at the rates of tests/tuner_model.py (2 MHz in, 5 kHz channel rate, 1 kHz
audio), WR_NCO_ROTATE with the audio ring on, blocks of 80 * D1 input frames; a second tuner of two receivers in two rate
groups; a twin of the first that is submitted the same blocks and never asked anything.

REFUSALS is the table: per reader and case the status and the words wr_last_error() holds.  The words are the entry
point's name where the message has always begun with it, and for the two refusals the readers share the words every
message has held: "several rate groups" and "nothing submitted".

A reader that refuses before it has bound the device and flushed must not send the last block's post stage out: under
WR_NCO_ROTATE that stage waits for the next submit, and its block is queued in the audio ring only when it goes.  So
wr_tuner_audio_ring_ready (and the ring's queue length) is 0 before and after wr_tuner_chan_spectra refuses a frame range
and wr_tuner_tones_push refuses a bank that is too small.  The third such refusal, the same submit pushed twice, can only
follow a push that was taken -- which flushed: the ring holds the block, ready is 1 before and after."""
import ctypes as C

import numpy as np
import pytest

import tuner_model
from webradio_amd import CTCSS_HZ, capi
from webradio_amd.device import Spectrum, ToneBank, Tuner

pytestmark = pytest.mark.gpu

OK, ARG, STATE = capi.WR_OK, capi.WR_ERR_ARG, capi.WR_ERR_STATE
FS, D1 = tuner_model.FS, tuner_model.D1
BLOCK = 80 * D1
K1, K2 = 80, 16
IFS = (-25_000 + 321, 321, 25_000 + 321)
N_FFT = tuner_model.CHAN_SPECTRUM_N

READERS = ("wr_chan_fetch", "wr_tuner_audio_dev", "wr_tuner_chan_spectra", "wr_tuner_chan_levels", "wr_tuner_tones_push",
           "wr_tuner_fetch_audio_all")
# case -> reader -> (status, words of wr_last_error(), None where the call is taken); a reader a case does not apply to is absent
REFUSALS = {
    "NULL tuner": {r: (ARG, r) for r in READERS},
    "NULL output": {r: (ARG, r) for r in READERS},
    "no such channel": {"wr_chan_fetch": (ARG, "wr_chan_fetch")},
    "not yet submitted": {
        "wr_chan_fetch": (STATE, "nothing submitted"),
        "wr_tuner_audio_dev": (OK, None),                       # (it shows where the audio will be)
        "wr_tuner_chan_spectra": (STATE, "nothing submitted"),
        "wr_tuner_chan_levels": (STATE, "nothing submitted"),
        "wr_tuner_tones_push": (STATE, "nothing submitted"),
        "wr_tuner_fetch_audio_all": (STATE, "nothing submitted"),
    },
    "several rate groups": {
        "wr_chan_fetch": (OK, None),                            # (a channel knows its group)
        "wr_tuner_audio_dev": (STATE, "several rate groups"),
        "wr_tuner_chan_spectra": (STATE, "several rate groups"),
        "wr_tuner_chan_levels": (STATE, "several rate groups"),
        "wr_tuner_tones_push": (STATE, "several rate groups"),
        "wr_tuner_fetch_audio_all": (STATE, "several rate groups"),
    },
}


class Asker:
    """calls a reader by name on a tuner handle (or None); `out=False`: its output (for the tone bank: the bank) is NULL"""

    def __init__(self, dev):
        self.dev, self.lib = dev, dev.lib
        self.spec = Spectrum(dev, N_FFT)
        self.bank = ToneBank(dev, 64, CTCSS_HZ, 1_000, 120)
        self.db = dev.malloc(64 * N_FFT * 4)
        self.buf = np.zeros(64 * 2 * K1, np.float32)
        self.n, self.stride, self.frames, self.slots = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint()

    def close(self):
        self.spec.destroy()
        self.bank.destroy()
        self.dev.free(self.db)

    def ask(self, reader, t, out=True, chan=0):
        lib, buf = self.lib, capi.ptr(self.buf)
        if reader == "wr_chan_fetch":
            return lib.wr_chan_fetch(t, chan, capi.WR_STAGE_AUDIO, buf if out else None, self.buf.size, C.byref(self.n))
        if reader == "wr_tuner_audio_dev":
            return lib.wr_tuner_audio_dev(t, C.byref(C.c_void_p()) if out else None, C.byref(self.stride), C.byref(self.frames))
        if reader == "wr_tuner_chan_spectra":
            return lib.wr_tuner_chan_spectra(t, self.spec.h, 0, C.c_void_p(self.db) if out else None, C.byref(self.slots))
        if reader == "wr_tuner_chan_levels":
            return lib.wr_tuner_chan_levels(t, buf if out else None, None, None, C.byref(self.frames), None, C.byref(self.slots))
        if reader == "wr_tuner_tones_push":
            return lib.wr_tuner_tones_push(t, self.bank.h if out else None, C.byref(self.slots))
        assert reader == "wr_tuner_fetch_audio_all"
        return lib.wr_tuner_fetch_audio_all(t, buf if out else None, self.buf.size, C.byref(self.stride), C.byref(self.frames),
                                            C.byref(self.slots))

    def holds(self, case, t, **how):
        for reader, (status, words) in REFUSALS[case].items():
            rc = self.ask(reader, t, **how)
            said = self.lib.wr_last_error().decode(errors="replace")
            print("%-20s %-26s -> %d %s" % (case, reader, rc, said if rc else ""))
            assert rc == status, (case, reader, rc, said)
            assert words is None or words in said, (case, reader, said)


def _tuner(dev):
    t = Tuner(dev, FS, len(IFS), BLOCK, capi.WR_NCO_ROTATE)
    chans = [t.add_receiver(f, tuner_model.CHAN_PASSBANDS[0], tuner_model.CHAN_RATE, (capi.WR_AM, capi.WR_FM, capi.WR_USB)[c],
                            tuner_model.AUDIO_PASSBAND, 1_000) for c, f in enumerate(IFS)]
    t.audio_ring(4)
    return t, chans


def _ring(t):
    """(wr_tuner_audio_ring_ready, blocks queued) once the device has gone idle: a block that was sent out has landed"""
    t.dev.sync()
    ready = C.c_int(-1)
    assert t.lib.wr_tuner_audio_ring_ready(t.h, C.byref(ready)) == OK
    return ready.value, t.ring_stats()[0]


def test_refusals_and_what_they_leave(dev):
    lib = dev.lib
    x = dev.upload(tuner_model.signal(2 * BLOCK, IFS[:2], seed=5))
    a = Asker(dev)
    t, chans = _tuner(dev)
    twin, _ = _tuner(dev)
    two = Tuner(dev, FS, 2, BLOCK, capi.WR_NCO_ROTATE)
    two.add_receiver(IFS[0], tuner_model.CHAN_PASSBANDS[0], 5_000, capi.WR_AM, tuner_model.AUDIO_PASSBAND, 1_000)
    two.add_receiver(IFS[2], tuner_model.CHAN_PASSBANDS[0], 10_000, capi.WR_AM, 2_000, 2_000)
    small = ToneBank(dev, 5, CTCSS_HZ, 1_000, 120)
    try:
        a.holds("NULL tuner", None)
        a.holds("not yet submitted", t.h)

        t.submit_device(x, BLOCK)
        twin.submit_device(x, BLOCK)
        # ---- refused before the flush: the block's post stage stays where it was
        assert _ring(t) == (0, 0)
        rc = lib.wr_tuner_chan_spectra(t.h, a.spec.h, K1 - N_FFT + 1, C.c_void_p(a.db), None)
        assert rc == ARG and b"reach beyond" in lib.wr_last_error()
        assert _ring(t) == (0, 0)
        assert lib.wr_tuner_tones_push(t.h, small.h, None) == ARG and b"64 channel slots" in lib.wr_last_error()
        assert _ring(t) == (0, 0)
        assert t.tones_push(a.bank) == 64                                  # taken: this one sends the post stage out
        assert _ring(t) == (1, 1)
        assert lib.wr_tuner_tones_push(t.h, a.bank.h, None) == STATE and b"in the bank already" in lib.wr_last_error()
        assert _ring(t) == (1, 1)
        assert list(a.bank.read()[3][:3]) == [K2] * 3                      # ... and nothing was counted twice

        a.holds("NULL output", t.h, out=False)
        for chan in (-1, len(chans), 1 << 20):
            a.holds("no such channel", t.h, chan=chan)
        out = np.zeros(K2, np.float32)
        assert lib.wr_chan_fetch(t.h, chans[0], capi.WR_STAGE_AUDIO, capi.ptr(out), out.size, None) == ARG
        assert b"wr_chan_fetch" in lib.wr_last_error()
        assert lib.wr_chan_slot(t.h, chans[0], None) == ARG and b"wr_chan_slot" in lib.wr_last_error()
        assert lib.wr_chan_slot(t.h, len(chans), C.byref(C.c_int())) == ARG and b"wr_chan_slot" in lib.wr_last_error()

        two.submit_device(x, BLOCK)
        a.holds("several rate groups", two.h)
        assert a.n.value == K2

        # ---- after all that the tuner makes the audio of a tuner that was never asked anything
        t.submit_device(x + 8 * BLOCK, BLOCK)
        twin.submit_device(x + 8 * BLOCK, BLOCK)
        got, want = t.fetch_audio_all(), twin.fetch_audio_all()
        assert got.shape == want.shape == (64, K2)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert all(np.abs(want[t.slot(ch)]).max() > 0 for ch in chans)
    finally:
        small.destroy()
        two.destroy()
        twin.destroy()
        t.destroy()
        a.close()
        dev.free(x)
