"""Thin Python handles over the C ABI: Device, Tuner (one FrontEnd's tuner with its
Receivers), Spectrum (SpectrumSink).  Used by tests, bench.py and the examples; the
arithmetic all happens in the HIP library.  Names follow the reference (radio.h:42-102).
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, ptr


def agc_design(target_dbfs=-12.0, decay_db_per_s=20.0, max_gain_db=60.0, audio_rate=10_000):
    """(target float32, floor_bits, step) of an AGC with these settings at this audio rate (wr_agc_design); needs no device."""
    target, floor_bits, step = C.c_float(), C.c_uint(), C.c_uint()
    check(capi.load().wr_agc_design(C.c_float(target_dbfs), C.c_float(decay_db_per_s), C.c_float(max_gain_db), audio_rate,
                                    C.byref(target), C.byref(floor_bits), C.byref(step)))
    return np.float32(target.value), floor_bits.value, step.value


class Device:
    """wr_dev: a gfx950 device + the HIP stream all work is issued on."""

    def __init__(self, index=0, stream=None):
        self.lib = capi.load()
        h = C.c_void_p()
        check(self.lib.wr_dev_open(C.byref(h), index, ptr(stream) if stream else None))
        self.h = h
        self.index = index

    def close(self):
        if self.h:
            self.lib.wr_dev_close(self.h)
            self.h = None

    def sync(self):
        check(self.lib.wr_dev_sync(self.h))

    # --- raw device memory for tests that do not want torch --------------------
    def malloc(self, nbytes):
        p = C.c_void_p()
        check(self.lib.wr_dev_malloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, p):
        check(self.lib.wr_dev_free(self.h, C.c_void_p(p)))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(max(arr.nbytes, 4))
        check(self.lib.wr_dev_upload(self.h, C.c_void_p(p), ptr(arr), arr.nbytes))
        return p

    def download(self, p, count, dtype=np.float32):
        out = np.empty(count, dtype=dtype)
        check(self.lib.wr_dev_download(self.h, ptr(out), C.c_void_p(p), out.nbytes))
        return out

    # --- one kernel per reference block -----------------------------------------
    def mix(self, iq, phase, phase_step):
        """DownConverter::process on a host array; returns (mixed, new_phase)."""
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        n = iq.size // 2
        din = self.upload(iq)
        dout = self.malloc(max(iq.nbytes, 4))
        ph = C.c_uint(phase)
        check(self.lib.wr_mix(self.h, C.c_void_p(din), C.c_void_p(dout), n, C.byref(ph), phase_step))
        out = self.download(dout, 2 * n)
        self.free(din)
        self.free(dout)
        return out, ph.value

    def fir_decimate(self, x, channels, decimation, coeff, history_dev):
        """LowPass::process on a host array; history_dev is a device pointer kept by the caller."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        nframes = x.size // channels
        nout = (nframes // decimation) * channels
        din = self.upload(x)
        dout = self.malloc(max(nout * 4, 4))
        coeff = np.ascontiguousarray(coeff, dtype=np.float32)     # its length is LowPass::_firLength
        check(self.lib.wr_fir_decimate_n(self.h, C.c_void_p(din), nframes, channels, decimation, coeff.size,
                                         ptr(coeff), C.c_void_p(history_dev), C.c_void_p(dout)))
        out = self.download(dout, nout)
        self.free(din)
        self.free(dout)
        return out

    def demod(self, mode, iq, prev):
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        n = iq.size // 2
        din = self.upload(iq)
        dout = self.malloc(max(n * 4, 4))
        prev = np.array(prev, dtype=np.float32)
        check(self.lib.wr_demod(self.h, mode, C.c_void_p(din), n, ptr(prev), C.c_void_p(dout)))
        out = self.download(dout, n)
        self.free(din)
        self.free(dout)
        return out, prev

    def iq_levels(self, p, nframes):
        """(mean, peak) of i*i + q*q over the [nframes][2] float array at device pointer p (wr_iq_levels), as
        numpy float32 scalars."""
        mean, peak = C.c_float(), C.c_float()
        check(self.lib.wr_iq_levels(self.h, C.c_void_p(p), nframes, C.byref(mean), C.byref(peak)))
        return np.float32(mean.value), np.float32(peak.value)

    def agc_rows(self, p, row_stride, nrows, nframes, target, floor_bits, step, state):
        """AGC in place on nrows rows of nframes floats at device pointer p, row_stride floats apart (wr_agc_rows): per row a
        target (float32), floor_bits, step (0xffffffff: no AGC on that row) and the state word; returns the new states."""
        target = np.ascontiguousarray(target, dtype=np.float32)
        floor_bits = np.ascontiguousarray(floor_bits, dtype=np.uint32)
        step = np.ascontiguousarray(step, dtype=np.uint32)
        state = np.array(state, dtype=np.uint32)
        assert target.size == floor_bits.size == step.size == state.size == nrows
        check(self.lib.wr_agc_rows(self.h, C.c_void_p(p), row_stride, nrows, nframes, ptr(target), ptr(floor_bits),
                                   ptr(step), ptr(state)))
        return state


class Tuner:
    """wr_tuner: every Receiver chain of one tuner, evaluated by one launch sequence."""

    def __init__(self, dev, input_rate, max_channels, max_block_frames, nco=capi.WR_NCO_ROTATE):
        self.dev = dev
        self.lib = dev.lib
        h = C.c_void_p()
        check(self.lib.wr_tuner_create(C.byref(h), dev.h, input_rate, max_channels, max_block_frames, nco))
        self.h = h
        self.input_rate = input_rate
        self.max_channels = max_channels

    def destroy(self):
        if self.h:
            self.lib.wr_tuner_destroy(self.h)
            self.h = None

    def add_receiver(self, if_hz, chan_passband, chan_rate, mode, audio_passband, audio_rate, fir_lengths=None,
                     stage2=None):
        """Receiver() + setFrontEnd(): the wiring of radio.cxx:62-90 with explicit parameters.
        fir_lengths: (channel, audio) LowPass::_firLength, powers of two: the channel filter up to 256
        (WR_FIR_FUSED_MAX; above 64: WR_NCO_EXACT the reference's own arithmetic, the other modes the ROTATE recurrence in L / 64 segments),
        the audio filter up to 256 as well (r05; default 64, 64).
        stage2: (fir_length, passband, out_rate) of a second channel LowPass in front of the demodulator; fir_length up to 256."""
        c = C.c_int()
        check(self.lib.wr_chan_add(self.h, C.byref(c)))
        ch = c.value
        check(self.lib.wr_chan_set_if(self.h, ch, if_hz))
        l1, l2 = fir_lengths if fir_lengths else (capi.WR_FIR_LENGTH, capi.WR_FIR_LENGTH)
        check(self.lib.wr_chan_set_filter_n(self.h, ch, 0, l1, chan_passband, chan_rate))
        if stage2:
            check(self.lib.wr_chan_set_filter_n(self.h, ch, 2, stage2[0], stage2[1], stage2[2]))
        check(self.lib.wr_chan_set_filter_n(self.h, ch, 1, l2, audio_passband, audio_rate))
        check(self.lib.wr_chan_set_mode(self.h, ch, mode))
        return ch

    def keep_stages(self, *stages):
        """Ask for intermediate stages (capi.WR_STAGE_DEMOD ...) to be kept for fetch()."""
        mask = 0
        for st in stages:
            mask |= 1 << st
        check(self.lib.wr_tuner_keep_stages(self.h, mask))

    def flush(self):
        """Launch a post stage (demod + audio filter) that is still waiting for the next submit."""
        check(self.lib.wr_tuner_flush(self.h))

    def blocks_per_launch(self, n):
        """Hold up to n back-to-back device blocks and launch them as one (the same bits, per group)."""
        check(self.lib.wr_tuner_set_blocks_per_launch(self.h, n))

    def streaming(self, enable=True):
        """Device blocks go to ONE persistent launch through a doorbell (wr_tuner_set_streaming): the same bits,
        no kernel launch per block.  flush() -- or anything else that touches the tuner -- closes the launch."""
        check(self.lib.wr_tuner_set_streaming(self.h, int(enable) if enable is not True else 1))

    def stream_info(self):
        """(live, launches opened, blocks taken) of the streaming mode"""
        live, launches, blocks = C.c_int(), C.c_ulonglong(), C.c_ulonglong()
        check(self.lib.wr_tuner_stream_info(self.h, C.byref(live), C.byref(launches), C.byref(blocks)))
        return bool(live.value), launches.value, blocks.value

    def stream_host_blocks(self):
        """blocks streamed out of page-locked host memory so far (wr_tuner_submit_u8(..., WR_HOST) while streaming)"""
        n = C.c_ulonglong()
        check(self.lib.wr_tuner_stream_host_blocks(self.h, C.byref(n)))
        return n.value

    def stream_long_blocks(self):
        """blocks (of launches that are over and checked) whose post stage ran in long runs of tiles: the host was ahead"""
        n = C.c_ulonglong()
        check(self.lib.wr_tuner_stream_long_blocks(self.h, C.byref(n)))
        return n.value

    def mark_launches(self, enable=True):
        """every launch that reads a submitted block stamps an event on completion (Ring.exchange_after waits for it)"""
        check(self.lib.wr_tuner_mark_launches(self.h, 1 if enable else 0))

    def seek(self, frame):
        """Every channel as if the stream started at `frame` (NCO phase closed-form): time sharding."""
        check(self.lib.wr_tuner_seek(self.h, C.c_ulonglong(frame)))

    def fetch_audio_all(self):
        """The last block's audio of every slot in one transfer: array [slots][frames]."""
        stride, frames, slots = C.c_size_t(), C.c_size_t(), C.c_uint()
        self.lib.wr_tuner_fetch_audio_all(self.h, None, 0, C.byref(stride), C.byref(frames), C.byref(slots))
        out = np.empty(max(1, slots.value * frames.value), dtype=np.float32)
        check(self.lib.wr_tuner_fetch_audio_all(self.h, ptr(out), out.size, C.byref(stride), C.byref(frames),
                                                C.byref(slots)))
        return out[: slots.value * frames.value].reshape(slots.value, frames.value)

    def slot(self, ch):
        s = C.c_int()
        check(self.lib.wr_chan_slot(self.h, ch, C.byref(s)))
        return s.value

    def audio_ring(self, depth):
        """Pinned host ring for the audio of every submit (0 = off)."""
        check(self.lib.wr_tuner_audio_ring(self.h, depth))

    def ring_acquire(self):
        """Oldest queued block: (audio[slots][frames] copy, seq).  Call ring_release() after."""
        p = C.POINTER(C.c_float)()
        stride, frames, slots, seq = C.c_size_t(), C.c_size_t(), C.c_uint(), C.c_ulonglong()
        check(self.lib.wr_tuner_audio_ring_acquire(self.h, C.byref(p), C.byref(stride), C.byref(frames),
                                                   C.byref(slots), C.byref(seq)))
        n = slots.value * stride.value
        a = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.float32)
        return a.reshape(slots.value, stride.value)[:, : frames.value], seq.value

    def ring_release(self):
        check(self.lib.wr_tuner_audio_ring_release(self.h))

    def ring_stats(self):
        q, o = C.c_uint(), C.c_ulonglong()
        check(self.lib.wr_tuner_audio_ring_stats(self.h, C.byref(q), C.byref(o)))
        return q.value, o.value

    def submit_count(self):
        """The number the next submit's ring entry will carry (submits numbered so far, failed ones too)."""
        n = C.c_ulonglong()
        check(self.lib.wr_tuner_submit_count(self.h, C.byref(n)))
        return n.value

    def remove_receiver(self, ch):
        check(self.lib.wr_chan_remove(self.h, ch))

    def set_if(self, ch, if_hz):
        check(self.lib.wr_chan_set_if(self.h, ch, if_hz))

    def set_af_gain(self, ch, gain_db):
        check(self.lib.wr_chan_set_af_gain(self.h, ch, C.c_float(gain_db)))

    def set_squelch(self, ch, threshold_dbfs, enable=True):
        check(self.lib.wr_chan_set_squelch(self.h, ch, C.c_float(threshold_dbfs), 1 if enable else 0))

    def set_agc(self, ch, target_dbfs=-12.0, decay_db_per_s=20.0, max_gain_db=60.0, enable=True):
        """The receiver's AGC (wr_chan_set_agc): peaks are brought to target_dbfs, the gain recovers at decay_db_per_s and
        never exceeds max_gain_db; from the next block on."""
        check(self.lib.wr_chan_set_agc(self.h, ch, C.c_float(target_dbfs), C.c_float(decay_db_per_s),
                                       C.c_float(max_gain_db), 1 if enable else 0))

    def get_agc(self, ch):
        """(enabled, target float32, floor_bits, step, state) as the last submit used and left them (wr_chan_get_agc)"""
        on, target = C.c_int(), C.c_float()
        floor_bits, step, state = C.c_uint(), C.c_uint(), C.c_uint()
        check(self.lib.wr_chan_get_agc(self.h, ch, C.byref(on), C.byref(target), C.byref(floor_bits), C.byref(step),
                                       C.byref(state)))
        return bool(on.value), np.float32(target.value), floor_bits.value, step.value, state.value

    def agc_info(self):
        """(receivers whose AGC the last submit ran, AGC kernel launches so far) (wr_tuner_agc_info)"""
        on, launches = C.c_uint(), C.c_ulonglong()
        check(self.lib.wr_tuner_agc_info(self.h, C.byref(on), C.byref(launches)))
        return on.value, launches.value

    def set_mode(self, ch, mode):
        check(self.lib.wr_chan_set_mode(self.h, ch, mode))

    def set_filter(self, ch, stage, passband, out_rate):
        check(self.lib.wr_chan_set_filter(self.h, ch, stage, passband, out_rate))

    def submit_host(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        check(self.lib.wr_tuner_submit(self.h, ptr(iq), iq.size // 2, capi.WR_HOST))
        self.dev.sync()   # the host array may be released by the caller

    def submit_device(self, dev_ptr, nframes):
        check(self.lib.wr_tuner_submit(self.h, ptr(dev_ptr), nframes, capi.WR_DEVICE))

    def submit_u8_host(self, raw):
        """A block in the RTL-SDR byte format in HOST memory (a numpy uint8 array, 2 bytes per frame)."""
        check(self.lib.wr_tuner_submit_u8(self.h, raw.ctypes.data_as(C.c_void_p), raw.size // 2, capi.WR_HOST))

    def last_staging(self):
        how = C.c_int()
        check(self.lib.wr_tuner_last_staging(self.h, C.byref(how)))
        return how.value

    def submit_u8_device(self, dev_ptr, nframes):
        """A block in the RTL-SDR byte format (io/rtlsdrtuner.cxx:106), already in device memory."""
        check(self.lib.wr_tuner_submit_u8(self.h, ptr(dev_ptr), nframes, capi.WR_DEVICE))

    def fetch(self, ch, stage, capacity):
        out = np.empty(max(capacity, 1), dtype=np.float32)
        n = C.c_size_t()
        check(self.lib.wr_chan_fetch(self.h, ch, stage, ptr(out), capacity, C.byref(n)))
        return out[: n.value].copy()

    def state(self, ch):
        ph = C.c_uint()
        prev = np.zeros(2, dtype=np.float32)
        check(self.lib.wr_chan_get_state(self.h, ch, C.byref(ph), ptr(prev)))
        return ph.value, prev

    def set_state(self, ch, phase, prev=None):
        p = None if prev is None else np.ascontiguousarray(prev, dtype=np.float32)
        check(self.lib.wr_chan_set_state(self.h, ch, phase, ptr(p)))

    def profile(self, enable):
        """False/0: off, True/1: every submit, n > 1: every n-th submit"""
        check(self.lib.wr_tuner_profile(self.h, int(enable)))

    def profile_read(self):
        """(launches, mean milliseconds) of the dominant kernel since the last read"""
        n = C.c_uint()
        ms = C.c_double()
        check(self.lib.wr_tuner_profile_read(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def audio_dev(self):
        a = C.c_void_p()
        stride = C.c_size_t()
        frames = C.c_size_t()
        check(self.lib.wr_tuner_audio_dev(self.h, C.byref(a), C.byref(stride), C.byref(frames)))
        return a.value, stride.value, frames.value

    def chan_spectra(self, spec, first_frame=0, db_dev=None):
        """Every receiver's CHANNEL spectrum in one launch (wr_tuner_chan_spectra): the dB row of channel-rate frames
        [first_frame, first_frame + spec.n) of the last submit, row of slot s at s * spec.n.  With db_dev (room for
        max_channels rounded up to 64 rows) the call is asynchronous and returns the rows written; without, it returns
        them as an array [slots][spec.n]."""
        slots = C.c_uint()
        if db_dev is not None:
            check(self.lib.wr_tuner_chan_spectra(self.h, spec.h, first_frame, ptr(db_dev), C.byref(slots)))
            return slots.value
        rows = (self.max_channels + 63) // 64 * 64
        p = self.dev.malloc(rows * spec.n * 4)
        try:
            check(self.lib.wr_tuner_chan_spectra(self.h, spec.h, first_frame, C.c_void_p(p), C.byref(slots)))
            out = self.dev.download(p, slots.value * spec.n)
        finally:
            self.dev.free(p)
        return out.reshape(slots.value, spec.n)

    def chan_levels(self):
        """Every receiver's signal level at the demodulator's input, from the last submit's channel IQ
        (wr_tuner_chan_levels): (mean, peak, muted, frames, audio_frames) -- mean and peak power (float32, full scale
        1.0) and the audio frames the squelch muted (uint32), arrays indexed by slot (Tuner.slot)."""
        rows = (self.max_channels + 63) // 64 * 64
        mean, peak = np.zeros(rows, np.float32), np.zeros(rows, np.float32)
        muted = np.zeros(rows, np.uint32)
        frames, audio_frames, slots = C.c_size_t(), C.c_size_t(), C.c_uint()
        check(self.lib.wr_tuner_chan_levels(self.h, ptr(mean), ptr(peak), ptr(muted), C.byref(frames),
                                            C.byref(audio_frames), C.byref(slots)))
        n = slots.value
        return mean[:n], peak[:n], muted[:n], frames.value, audio_frames.value

    def tones_push(self, bank):
        """The last submit's audio rows of every channel slot into a ToneBank (wr_tuner_tones_push); row = Tuner.slot.
        Returns the rows pushed (whole lane groups of 64)."""
        slots = C.c_uint()
        check(self.lib.wr_tuner_tones_push(self.h, bank.h, C.byref(slots)))
        return slots.value

    def dcs_push(self, bank):
        """The last submit's audio rows of every channel slot into a DcsBank (wr_tuner_dcs_push); row = Tuner.slot.
        Returns the rows pushed (whole lane groups of 64)."""
        slots = C.c_uint()
        check(self.lib.wr_tuner_dcs_push(self.h, bank.h, C.byref(slots)))
        return slots.value

    def resamp_push(self, rs):
        """The last submit's audio rows of every channel slot through a Resampler (wr_tuner_resamp_push); row = Tuner.slot.
        Returns the output frames as an array [slots][n_out] (slots: whole lane groups of 64), downloaded."""
        rows = (self.max_channels + 63) // 64 * 64
        _, _, frames = self.audio_dev()
        stride = max(rs.out_frames(frames), 1)
        p = self.dev.malloc(rows * stride * 4)
        try:
            n_out, slots = C.c_size_t(), C.c_uint()
            check(self.lib.wr_tuner_resamp_push(self.h, rs.h, C.c_void_p(p), stride, C.byref(n_out), C.byref(slots)))
            out = self.dev.download(p, slots.value * stride)
        finally:
            self.dev.free(p)
        return out.reshape(slots.value, stride)[:, : n_out.value].copy()

    def voice_push(self, bank, out, out_stride):
        """The last submit's audio rows of every channel slot through a VoiceBank (wr_tuner_voice_push); row = Tuner.slot.
        Row s's frames go to `out` (a device pointer or a torch tensor) + s * out_stride floats.  Returns the rows pushed
        (whole lane groups of 64).  Asynchronous."""
        slots = C.c_uint()
        check(self.lib.wr_tuner_voice_push(self.h, bank.h, ptr(out), out_stride, C.byref(slots)))
        return slots.value


def tone_step(hz, audio_rate):
    """a tone's phase step per audio frame, llround(hz / audio_rate * 2^32) (wr_tone_step); needs no device."""
    step = C.c_uint()
    check(capi.load().wr_tone_step(C.c_double(hz), audio_rate, C.byref(step)))
    return step.value


class ToneBank:
    """wr_tones: up to 64 tone correlators per row, integrated over windows of `window` audio frames that run on from
    push to push (include/webradio_amd.h: TONE BANK)."""

    def __init__(self, dev, max_rows, tones_hz, audio_rate, window, steps=None):
        """tones_hz at audio_rate -- or, with `steps`, the phase steps themselves (tones_hz and audio_rate are then ignored)"""
        self.dev = dev
        self.lib = dev.lib
        self.max_rows = max_rows
        self.window = window
        if steps is None:
            steps = [tone_step(hz, audio_rate) for hz in tones_hz]
        self.steps = np.array(steps, dtype=np.uint32)
        self.ntones = self.steps.size
        h = C.c_void_p()
        check(self.lib.wr_tones_create(C.byref(h), dev.h, max_rows, ptr(self.steps), self.ntones, window))
        self.h = h

    def destroy(self):
        if self.h:
            self.lib.wr_tones_destroy(self.h)
            self.h = None

    def reset(self, row=-1):
        """a row (every row: row < 0) begins a new stream -- after Tuner.seek, a history reset or a retune"""
        check(self.lib.wr_tones_reset(self.h, row))

    def push_rows(self, p, row_stride, nrows, nframes):
        """nrows rows of nframes floats at device pointer p, row_stride floats apart, continue rows 0 .. nrows-1"""
        check(self.lib.wr_tones_push_rows(self.h, C.c_void_p(p), row_stride, nrows, nframes))

    def read(self):
        """(iq int64 [rows][ntones][2], energy int64 [rows], windows uint64 [rows], fill uint32 [rows]): the last complete
        window's I, Q and E, the windows so far and the frames in the open one (wr_tones_read); waits for the device."""
        iq = np.zeros((self.max_rows, self.ntones, 2), np.int64)
        energy = np.zeros(self.max_rows, np.int64)
        windows = np.zeros(self.max_rows, np.uint64)
        fill = np.zeros(self.max_rows, np.uint32)
        rows = C.c_uint()
        check(self.lib.wr_tones_read(self.h, ptr(iq), ptr(energy), ptr(windows), ptr(fill), C.byref(rows)))
        assert rows.value == self.max_rows
        return iq, energy, windows, fill

    def ratios(self):
        """rho[rows][ntones] = 2 (I^2 + Q^2) / (W E 2^14) in float64: the share of the last complete window's audio power
        that sits in each tone; 0 where E is 0"""
        iq, energy, _, _ = self.read()
        return ratios(iq, energy, self.window)


def ratios(iq, energy, window):
    i, q = iq[..., 0].astype(np.float64), iq[..., 1].astype(np.float64)
    den = float(window) * energy.astype(np.float64) * 16384.0
    out = np.zeros(i.shape, np.float64)
    np.divide(2.0 * (i * i + q * q), den[..., None], out=out, where=den[..., None] > 0)
    return out


def dcs_word(code):
    """the 23-bit Golay word of a DCS code (0o023: dcs_word(0o023)), bit 0 sent first (wr_dcs_word); needs no device."""
    word = C.c_uint()
    check(capi.load().wr_dcs_word(code, C.byref(word)))
    return word.value


def dcs_step(audio_rate):
    """134.4 bit/s in units of 2^-32 bit per audio frame (wr_dcs_step); needs no device."""
    step = C.c_uint()
    check(capi.load().wr_dcs_step(audio_rate, C.byref(step)))
    return step.value


class DcsBank:
    """wr_dcs: up to 128 DCS code words tried on every row at every bit, in both polarities, the streams running on from
    push to push on one clock (include/webradio_amd.h: DCS BANK)."""

    def __init__(self, dev, max_rows, codes, audio_rate, max_errors=0, words=None):
        """codes (ints: 0o023 ...) at audio_rate -- or, with `words`, the 23-bit words themselves (codes is then ignored)"""
        self.dev = dev
        self.lib = dev.lib
        self.max_rows = max_rows
        if words is None:
            words = [dcs_word(code) for code in codes]
        self.words = np.array(words, dtype=np.uint32)
        self.ncodes = self.words.size
        self.step = dcs_step(audio_rate)
        self.max_errors = max_errors
        h = C.c_void_p()
        check(self.lib.wr_dcs_create(C.byref(h), dev.h, max_rows, ptr(self.words), self.ncodes, self.step, max_errors))
        self.h = h

    def destroy(self):
        if self.h:
            self.lib.wr_dcs_destroy(self.h)
            self.h = None

    def reset(self, row=-1):
        """a row begins a new stream, the clock runs on (row < 0: every row, and the clock returns to 0)"""
        check(self.lib.wr_dcs_reset(self.h, row))

    def seek(self, frame):
        """every row begins a new stream with the clock at `frame`"""
        check(self.lib.wr_dcs_seek(self.h, frame))

    def push_rows(self, p, row_stride, nrows, nframes):
        """nrows rows of nframes floats at device pointer p, row_stride floats apart, continue rows 0 .. nrows-1"""
        check(self.lib.wr_dcs_push_rows(self.h, C.c_void_p(p), row_stride, nrows, nframes))

    def read(self):
        """(agree uint8 [rows][ncodes][2], run uint32 [rows][ncodes][2], hits uint64 [rows][ncodes][2], evals uint64 [rows]):
        the last evaluation's agreeing bits per code as sent ([..., 0]) and inverted ([..., 1]), the matches in a row up
        to it, all matches and the evaluations so far (wr_dcs_read); waits for the device."""
        agree = np.zeros((self.max_rows, self.ncodes, 2), np.uint8)
        run = np.zeros((self.max_rows, self.ncodes, 2), np.uint32)
        hits = np.zeros((self.max_rows, self.ncodes, 2), np.uint64)
        evals = np.zeros(self.max_rows, np.uint64)
        rows = C.c_uint()
        check(self.lib.wr_dcs_read(self.h, ptr(agree), ptr(run), ptr(hits), ptr(evals), C.byref(rows)))
        assert rows.value == self.max_rows
        return agree, run, hits, evals

    def info(self):
        """(ncodes, step, max_errors, frames)"""
        n, step, me, frames = C.c_uint(), C.c_uint(), C.c_uint(), C.c_ulonglong()
        check(self.lib.wr_dcs_info(self.h, C.byref(n), C.byref(step), C.byref(me), C.byref(frames)))
        return n.value, step.value, me.value, frames.value


# wr_detection: a record of Spectrum.rows_detect
DETECTION = np.dtype([("first", np.uint32), ("last", np.uint32), ("peak_bin", np.uint32), ("hot", np.uint32),
                      ("peak", np.float32), ("floor", np.float32)])


def bin_hz(fft_size, sample_rate, centre_hz, bin):
    """centre_hz + (bin - fft_size / 2) * sample_rate / fft_size (wr_spectrum_bin_hz); needs no device"""
    hz = C.c_double()
    check(capi.load().wr_spectrum_bin_hz(fft_size, sample_rate, centre_hz, bin, C.byref(hz)))
    return hz.value


class Spectrum:
    """wr_spectrum: SpectrumSink (io/spectrumsink.h:44-68).  real=True: one float per frame (a receiver's audio),
    wr_spectrum_create_real -- pushes and batches then count samples."""

    def __init__(self, dev, fft_size, hop=0, real=False):
        self.dev = dev
        self.lib = dev.lib
        self.n = fft_size
        self.ch = 1 if real else 2
        h = C.c_void_p()
        create = self.lib.wr_spectrum_create_real if real else self.lib.wr_spectrum_create
        check(create(C.byref(h), dev.h, fft_size, hop))
        self.h = h

    def destroy(self):
        if self.h:
            self.lib.wr_spectrum_destroy(self.h)
            self.h = None

    def push_host(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        check(self.lib.wr_spectrum_push(self.h, ptr(iq), iq.size // self.ch, capi.WR_HOST))

    def push_device(self, dev_ptr, nframes):
        check(self.lib.wr_spectrum_push(self.h, ptr(dev_ptr), nframes, capi.WR_DEVICE))

    def get_db(self):
        out = np.empty(self.n, dtype=np.float32)
        check(self.lib.wr_spectrum_get_db(self.h, ptr(out)))
        return out

    def get_bins(self):
        out = np.empty(2 * self.n, dtype=np.float32)
        check(self.lib.wr_spectrum_get_bins(self.h, ptr(out)))
        return out

    def waterfall_row(self, width, hold=0):
        db = np.empty(width, dtype=np.float32)
        pal = np.empty(width, dtype=np.uint8)
        check(self.lib.wr_spectrum_get_waterfall_row(self.h, width, hold, ptr(db), ptr(pal)))
        return db, pal

    def frames_done(self):
        n = C.c_ulong()
        check(self.lib.wr_spectrum_frames_done(self.h, C.byref(n)))
        return n.value

    def lazy_info(self):
        """(pushes kept for later because a streaming launch was open, frames transformed on demand)"""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        check(self.lib.wr_spectrum_lazy_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def batch_db(self, iq_dev, nframes_fft, db_dev):
        check(self.lib.wr_spectrum_batch_db(self.h, ptr(iq_dev), nframes_fft, ptr(db_dev)))

    def batch_db_rows(self, in_dev, row_stride, nrows, db_dev):
        """dB rows of the first fft_size frames of `nrows` rows lying `row_stride` frames apart in device memory"""
        check(self.lib.wr_spectrum_batch_db_rows(self.h, ptr(in_dev), row_stride, nrows, ptr(db_dev)))

    def batch_avg(self, in_dev, nframes_fft, mean_dev=None, peak_dev=None, ngroups=1, group_stride=0, linear=False):
        """mean and peak-hold rows over the `nframes_fft` frames of each of `ngroups` groups lying `group_stride` frames
        apart in device memory (wr_spectrum_batch_avg): dB, or the powers themselves with `linear`"""
        check(self.lib.wr_spectrum_batch_avg(self.h, ptr(in_dev), nframes_fft, ngroups, group_stride, int(bool(linear)),
                                             ptr(mean_dev), ptr(peak_dev)))

    def rows_waterfall(self, db_dev, nrows, width, hold, db_rows_dev=None, palette_dev=None):
        """`nrows` shifted dB rows in device memory to pixel rows of `width` columns (wr_spectrum_rows_waterfall)"""
        check(self.lib.wr_spectrum_rows_waterfall(self.h, ptr(db_dev), nrows, width, int(hold), ptr(db_rows_dev),
                                                  ptr(palette_dev)))

    def channels(self):
        c = C.c_uint()
        check(self.lib.wr_spectrum_channels(self.h, C.byref(c)))
        return c.value

    def detect_rule(self, **fields):
        """wr_detect_rule_default for this spectrum's size, with `fields` (bin0, nbins, span, percent, threshold, linear,
        max_gap, min_width) set over it; a window given without a span gets one that divides it"""
        rule = capi.DetectRule()
        check(self.lib.wr_detect_rule_default(self.n, C.byref(rule)))
        for k, v in fields.items():
            if k not in dict(capi.DetectRule._fields_):
                raise TypeError("wr_detect_rule has no field %r" % k)
            setattr(rule, k, v)
        if "nbins" in fields and "span" not in fields and rule.nbins % rule.span:
            rule.span = rule.nbins
        return rule

    def rows_detect(self, rows_dev, nrows, rule, max_det, det_dev, count_dev, floor_dev=None):
        """noise floors and occupied segments of `nrows` rows of fft_size floats in device memory (wr_spectrum_rows_detect):
        count_dev[nrows], det_dev[nrows][max_det] records of DETECTION, floor_dev[nrows][nbins / span] if given.  Async."""
        check(self.lib.wr_spectrum_rows_detect(self.h, ptr(rows_dev), nrows, C.byref(rule), max_det, ptr(det_dev),
                                               ptr(count_dev), ptr(floor_dev)))

    def detect(self, rows_dev, nrows, max_det=64, **rule_fields):
        """rows_detect with everything allocated, waited for and downloaded: (records, counts, floors) -- a list of one
        DETECTION array per row, cut to min(count, max_det); the counts [nrows]; the floors [nrows][nbins / span]"""
        rule = self.detect_rule(**rule_fields)
        nspans = rule.nbins // rule.span if rule.span else 1     # (a span of 0 is the call's to refuse)
        dev = self.dev
        bufs = [dev.malloc(max(1, nrows * max_det) * DETECTION.itemsize), dev.malloc(max(1, nrows) * 4),
                dev.malloc(max(1, nrows * nspans) * 4)]
        try:
            self.rows_detect(rows_dev, nrows, rule, max_det, bufs[0], bufs[1], bufs[2])
            dev.sync()
            det = dev.download(bufs[0], nrows * max_det, DETECTION).reshape(nrows, max_det)
            counts = dev.download(bufs[1], nrows, np.uint32)
            floors = dev.download(bufs[2], nrows * nspans).reshape(nrows, nspans)
        finally:
            for b in bufs:
                dev.free(b)
        return [det[r, : min(int(counts[r]), max_det)].copy() for r in range(nrows)], counts, floors

    def bin_hz(self, sample_rate, centre_hz, bin):
        """the frequency of (fractional) bin `bin` of a shifted row of this size (wr_spectrum_bin_hz)"""
        return bin_hz(self.n, sample_rate, centre_hz, bin)


class Ring:
    """wr_ring: the halo ring of a time-sharded stream (BASELINE config 5) on RCCL -- one
    ncclSend / ncclRecv pair per exchange, on its own stream, handed to the device's stream by
    events.  `id_bytes`: what rank 0's Ring.make_id() returned, brought to every rank by the host."""

    @staticmethod
    def make_id():
        lib = capi.load()
        buf = (C.c_ubyte * lib.wr_ring_id_bytes())()
        check(lib.wr_ring_make_id(buf, len(buf)))
        return bytes(buf)

    @staticmethod
    def rccl_version():
        v = C.c_int()
        check(capi.load().wr_ring_version(C.byref(v)))
        return v.value

    def __init__(self, dev, id_bytes, rank, world):
        self.lib = capi.load()
        h = C.c_void_p()
        buf = (C.c_ubyte * len(id_bytes)).from_buffer_copy(id_bytes)
        check(self.lib.wr_ring_create(C.byref(h), dev.h, buf, len(id_bytes), rank, world))
        self.h, self.rank, self.world = h, rank, world

    def exchange(self, send_dev, recv_dev, nfloats):
        """enqueue: send_dev -> rank + 1, recv_dev <- rank - 1 (device pointers or torch tensors)"""
        check(self.lib.wr_ring_exchange(self.h, ptr(send_dev), ptr(recv_dev), nfloats))

    def exchange_after(self, tuner, send_dev, recv_dev, nfloats):
        """the same, ordered behind the tuner's launches so far (Tuner.mark_launches(True)) instead of behind the
        device's stream: for a halo that is input, received into a buffer only the tuner reads"""
        check(self.lib.wr_ring_exchange_after(self.h, tuner.h, ptr(send_dev), ptr(recv_dev), nfloats))

    def wait(self):
        """the device's stream waits for the last exchange (no host wait)"""
        check(self.lib.wr_ring_wait(self.h))

    def exchanges(self):
        n = C.c_ulonglong()
        check(self.lib.wr_ring_info(self.h, None, None, C.byref(n)))
        return n.value

    def destroy(self):
        if self.h:
            self.lib.wr_ring_destroy(self.h)
            self.h = None


def resamp_ratio(in_rate, out_rate):
    """(L, M): out_rate / in_rate in lowest terms (wr_resamp_ratio); needs no device."""
    L, M = C.c_uint(), C.c_uint()
    check(capi.load().wr_resamp_ratio(in_rate, out_rate, C.byref(L), C.byref(M)))
    return L.value, M.value


def resamp_design(in_rate, out_rate, taps_per_phase=32):
    """(taps float32 [L][P], L, M): the Kaiser-windowed sinc of wr_resamp_design; needs no device."""
    L, M = resamp_ratio(in_rate, out_rate)
    taps = np.zeros((L, max(taps_per_phase, 1)), np.float32)
    check(capi.load().wr_resamp_design(in_rate, out_rate, taps_per_phase, ptr(taps), None, None))
    return taps, L, M


class Resampler:
    """wr_resamp: max_rows rows of audio resampled by one ratio L / M = out_rate / in_rate with a polyphase FIR of
    taps_per_phase taps per phase, the streams running on from push to push (include/webradio_amd.h: RESAMPLER)."""

    def __init__(self, dev, max_rows, in_rate, out_rate, taps_per_phase=32, taps=None):
        """wr_resamp_design's taps -- or, with `taps` [L][P], the caller's own for the same ratio"""
        self.dev = dev
        self.lib = dev.lib
        self.max_rows = max_rows
        if taps is None:
            taps, self.L, self.M = resamp_design(in_rate, out_rate, taps_per_phase)
        else:
            self.L, self.M = resamp_ratio(in_rate, out_rate)
            taps = np.ascontiguousarray(taps, dtype=np.float32)
            assert taps.ndim == 2 and taps.shape[0] == self.L
        self.taps = taps
        self.P = taps.shape[1]
        h = C.c_void_p()
        check(self.lib.wr_resamp_create(C.byref(h), dev.h, max_rows, self.L, self.M, self.P, ptr(self.taps)))
        self.h = h

    def destroy(self):
        if self.h:
            self.lib.wr_resamp_destroy(self.h)
            self.h = None

    def reset(self, row=-1):
        """a row's history is cleared (row < 0: every row's, and the clock returns to 0)"""
        check(self.lib.wr_resamp_reset(self.h, row))

    def out_frames(self, nframes):
        """the output frames a push of nframes would yield now"""
        n = C.c_size_t()
        check(self.lib.wr_resamp_out_frames(self.h, nframes, C.byref(n)))
        return n.value

    def push_rows(self, p, row_stride, nrows, nframes, out_p, out_stride):
        """nrows rows of nframes floats at device pointer p, row_stride floats apart, continue rows 0 .. nrows-1; row r's
        output frames go to device pointer out_p + 4 * r * out_stride.  Returns their number.  Asynchronous."""
        n = C.c_size_t()
        check(self.lib.wr_resamp_push_rows(self.h, C.c_void_p(p), row_stride, nrows, nframes, C.c_void_p(out_p), out_stride,
                                           C.byref(n)))
        return n.value

    def info(self):
        """(L, M, P, frames_in, frames_out)"""
        L, M, P, fi, fo = C.c_uint(), C.c_uint(), C.c_uint(), C.c_ulonglong(), C.c_ulonglong()
        check(self.lib.wr_resamp_info(self.h, C.byref(L), C.byref(M), C.byref(P), C.byref(fi), C.byref(fo)))
        return L.value, M.value, P.value, fi.value, fo.value


def voice_design(audio_rate, taps, highpass_hz=300, lowpass_hz=3000, deemph_us=0):
    """float32 [taps]: the linear-phase voice filter of wr_voice_design -- a band-pass (an edge of 0: none) with de-emphasis
    (0: none), its group delay taps / 2 - 1 frames; needs no device."""
    out = np.zeros(max(taps, 1), np.float32)
    check(capi.load().wr_voice_design(audio_rate, taps, highpass_hz, lowpass_hz, deemph_us, ptr(out)))
    return out


class VoiceBank:
    """wr_voice: max_rows rows of audio, each through one of up to 16 FIR filters of one length T or muted, the streams
    running on from push to push (include/webradio_amd.h: VOICE BANK).  A row's control word is its filter index, plus
    VoiceBank.MUTE."""

    MUTE = 0x100

    def __init__(self, dev, max_rows, taps):
        """`taps`: [F][T], or [T] for a single filter"""
        self.dev = dev
        self.lib = dev.lib
        self.max_rows = max_rows
        self.taps = np.atleast_2d(np.ascontiguousarray(taps, dtype=np.float32))
        assert self.taps.ndim == 2
        self.F, self.T = self.taps.shape
        h = C.c_void_p()
        check(self.lib.wr_voice_create(C.byref(h), dev.h, max_rows, self.T, self.F, ptr(self.taps)))
        self.h = h

    def destroy(self):
        if self.h:
            self.lib.wr_voice_destroy(self.h)
            self.h = None

    def reset(self, row=-1):
        """a row's history is cleared (row < 0: every row's, and the frame count returns to 0); the control words stay"""
        check(self.lib.wr_voice_reset(self.h, row))

    def set_rows(self, first, words):
        """the control words of rows first, first + 1, ...: all of them or, if one is refused, none"""
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        check(self.lib.wr_voice_set_rows(self.h, first, words.size, ptr(words)))

    def get_rows(self, first=0, n=None):
        words = np.zeros(self.max_rows - first if n is None else n, np.uint32)
        check(self.lib.wr_voice_get_rows(self.h, first, words.size, ptr(words)))
        return words

    def push_rows(self, p, row_stride, nrows, nframes, out_p, out_stride):
        """nrows rows of nframes floats at device pointer p, row_stride floats apart, continue rows 0 .. nrows-1; row r's
        nframes output frames go to device pointer out_p + 4 * r * out_stride.  Asynchronous."""
        check(self.lib.wr_voice_push_rows(self.h, C.c_void_p(p), row_stride, nrows, nframes, C.c_void_p(out_p), out_stride))

    def info(self):
        """(T, F, frames)"""
        T, F, frames = C.c_uint(), C.c_uint(), C.c_ulonglong()
        check(self.lib.wr_voice_info(self.h, C.byref(T), C.byref(F), C.byref(frames)))
        return T.value, F.value, frames.value
