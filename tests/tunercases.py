"""What the tests of the fused per-tuner path (wr_tuner_*) share: the tolerances, the oracle's chain with explicit filter
lengths, bit views, the ring drain, and one receiver through the HIP path block by block or through the streaming launch.
(numpy and ctypes only: a CPU test may import it.)

Tolerances (float32, |x| <= 1):
  WR_NCO_EXACT  channel-filter IQ is BIT-EXACT (same table, same unfused operations in the
                same order); AM/USB/LSB demod and audio bit-exact; FM within FM_ATOL.
  WR_NCO_SPLIT  the LO comes from the two-level table: it differs from the reference's
                table entry by <= 3.5e-7 (the reference table itself carries 2.4e-7 of
                argument-rounding noise) and the taps are accumulated with FMAs, so
                channel IQ is within IQ_ATOL = 1e-6 absolute; FM audio on channels
                that hold a carrier within AUDIO_ATOL = 1e-5, and on EVERY channel -- noise-only
                ones too, where FM is ill-conditioned -- within what the channel's
                own IQ difference allows: per demod frame 1.25 * (|dz[k]|/|z[k]| + |dz[k-1]|/|z[k-1]|)
                / (2 pi) + 2.4e-7 cycles, through the audio filter's |taps| (tests/fm_bound.py;
                the bound itself is tested on the CPU in tests/test_fm_bound.py).
  WR_NCO_ROTATE (default) the same table index per frame; each LO value is the anchor's turned
                by a product of correctly rounded turns (Horner recurrence): same tolerances as
                SPLIT, measured 1.3e-7 on channel IQ.  AM / USB / LSB audio: |.| and the sums of Re and Im are
                2-Lipschitz in the channel IQ, then the linear audio filter -- LINEAR_ATOL = 2e-6 per unit of sum|h2|.
In every mode the integer NCO phase is exact and a frame's bits do not depend on how the stream
is cut into blocks."""
import numpy as np

from fm_bound import FM_ATOL  # noqa: F401  (2.4e-7: the in-kernel atan2 against glibc's; stated where the FM bound is derived)
from webradio_amd import capi
from webradio_amd.device import Tuner

IQ_ATOL = 1e-6
AUDIO_ATOL = 1e-5
LINEAR_ATOL = 2e-6


def bits(a):
    """the array's own 32-bit words (a float32 array: nothing is converted on the way)"""
    return np.ascontiguousarray(a).view(np.uint32)


def bits_f32(a):
    """the 32-bit words of the values as float32: for scalars, lists and arrays of another type"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def drain(t, count):
    """the next `count` entries of the tuner's audio ring: [(sequence number, audio rows)]"""
    out = []
    for b in range(count):
        audio, seq = t.ring_acquire()
        out.append((seq, audio.copy()))
        t.ring_release()
    return out


class OracleChain:
    """A Receiver chain assembled from the oracle's blocks with explicit filter lengths:
    mixer -> LowPass(L1, D1) [-> LowPass(L1b, D1b)] -> demodulator -> LowPass(L2, D2).
    taps: {"channel" / "second" / "audio": coefficients} in place of that stage's LowPass design (wr_chan_set_taps_n).
    keep_history: over blocks of several sizes the filters keep their true histories (wr_oracle.fir_keep_history; the
    reference's LowPass loses them when the size changes, quirk Q7, which the product deliberately does not copy)."""

    def __init__(self, oracle, fs, if_hz, l1, pb1, d1, mode, l2, pb2, d2, stage2=None, taps=None, keep_history=False):
        taps = taps or {}
        self.o, self.mode, self.keep_history = oracle, mode, keep_history
        self.table = oracle.sin_table()
        self.step = oracle.phase_step(if_hz, fs)
        self.phase = 0
        self.prev = (0.0, 0.0)
        self.f1 = oracle.Fir(2, d1, taps.get("channel", oracle.lowpass_design(pb1, fs, l1)))
        r = fs // d1
        self.f1b = None
        if stage2:
            l1b, pb1b, d1b = stage2
            self.f1b = oracle.Fir(2, d1b, taps.get("second", oracle.lowpass_design(pb1b, r, l1b)))
            r //= d1b
        self.f2 = oracle.Fir(1, d2, taps.get("audio", oracle.lowpass_design(pb2, r, l2)))

    def run(self, iq):
        if self.keep_history:
            n = np.asarray(iq).size // 2
            self.o.fir_keep_history(self.f1.s, 2 * n)
            k = n // self.f1.decimation
            if self.f1b is not None:
                self.o.fir_keep_history(self.f1b.s, 2 * k)
                k //= self.f1b.decimation
            self.o.fir_keep_history(self.f2.s, k)
        mixed, self.phase = self.o.mix(self.table, self.phase, self.step, iq)
        c = self.f1.process(mixed)
        if self.f1b is not None:
            c = self.f1b.process(c)
        d, self.prev = self.o.demod(self.mode, self.prev, c)
        return self.f2.process(d), c, d


# ---- one receiver of tests/refcases.py (c: a case of refcases.CHAINS) through the HIP path ------------------------------------

def hip_chain(dev, c, iq, nco):
    """a launch per block, every stage kept: (audio, channel IQ, demodulator output) of the whole stream"""
    t = Tuner(dev, c["fs"], 1, c["block"], nco)
    ch = t.add_receiver(c["if_hz"], c["cpb"], c["crate"], c["mode"], c["apb"], c["arate"])
    t.keep_stages(capi.WR_STAGE_DEMOD)
    n = c["block"]
    audio, chan, dem = [], [], []
    for b in range(c["blocks"]):
        t.submit_host(iq[2 * n * b: 2 * n * (b + 1)])
        chan.append(t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * n))
        dem.append(t.fetch(ch, capi.WR_STAGE_DEMOD, n))
        audio.append(t.fetch(ch, capi.WR_STAGE_AUDIO, n))
    t.destroy()
    return np.concatenate(audio), np.concatenate(chan), np.concatenate(dem)


def stream_cut(c):
    """The block size a streaming launch takes (wr_tuner_set_streaming: at least 64 channel-rate frames, whole audio
    frames per block): the case's own where that qualifies, otherwise consecutive blocks merged -- a frame's bits do not
    depend on where the stream is cut into blocks (lowpass.cxx:138-142 carries the history over)."""
    d1, d2 = c["fs"] // c["crate"], c["crate"] // c["arate"]
    for m in range(1, c["blocks"] + 1):
        n = c["block"] * m
        if c["blocks"] % m == 0 and n >= 64 * d1 and n % (d1 * d2) == 0:
            return n
    raise AssertionError("no cut of this case is eligible for a streaming launch")


def hip_chain_stream(dev, c, iq):
    """The same Receiver through k_tuner_stream -- the kernel bench.py times: the input resident in device memory,
    Tuner.streaming(True), one submit_device per block (the first opens the launch, the others ring its doorbell), the
    audio of EVERY block out of the pinned ring, the last block's channel IQ.  Asserts that the launch was live and took
    every block (no silent fall-back to a launch per block)."""
    import torch
    n = stream_cut(c)
    nblk = c["block"] * c["blocks"] // n
    x = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
    torch.cuda.synchronize()
    t = Tuner(dev, c["fs"], 1, n, capi.WR_NCO_ROTATE)
    ch = t.add_receiver(c["if_hz"], c["cpb"], c["crate"], c["mode"], c["apb"], c["arate"])
    t.audio_ring(nblk)
    t.streaming(True)
    for b in range(nblk):
        t.submit_device(x[2 * n * b: 2 * n * (b + 1)], n)
    info = t.stream_info()
    assert info == (True, 1, nblk), "stream_info() %s behind %d blocks of %d frames: not one live launch" % (info, nblk, n)
    t.flush()
    info = t.stream_info()
    assert info[0] is False, "stream_info() %s: the launch is still live behind a flush" % (info,)
    slot, audio = t.slot(ch), []
    for b, (seq, a) in enumerate(drain(t, nblk)):
        assert seq == b, "ring entry %d has sequence number %d" % (b, seq)
        audio.append(a[slot])
    chan_last = t.fetch(ch, capi.WR_STAGE_CHAN_IQ, 2 * n)
    t.destroy()
    del x
    return np.concatenate(audio), chan_last
