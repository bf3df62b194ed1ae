"""-m gpu: wr_spectrum_batch_avg (mean and peak-hold rows over all frames of a block) and wr_spectrum_rows_waterfall.

Two yardsticks (tests/specavg_np.py).  To the bit, with linear rows, on the sizes one workgroup transforms: the rule
restated in float32 numpy on the bins a second Spectrum gives for each frame pushed on its own.  In dB, on every path and
every bin: the float64 reference -- oracle.spectrum_np per frame, averaged or maximised as powers -- under the mask and
share check of tests/test_gpu_spectrum_all_bins.py with DB_ATOL of tests/speccases.py, unchanged: every frame's row
is held to it already, a mean of such rows is no further off, and the order of summation adds under 1e-4 dB at 259
frames (tests/test_spectrum_avg_reference.py prints that figure).  Every check prints the figures it then asserts on."""
import ctypes as C

import numpy as np
import pytest

import specavg_np as sa
from flat_spectrum import MASK_OUT_SHARE
from speccases import DB_ATOL
from tunercases import bits_f32
from webradio_amd import capi, synth
from webradio_amd.device import Spectrum, Tuner

pytestmark = pytest.mark.gpu


def _say(what, n, **figures):
    print("spectrum-avg: %-30s n=%-8d %s" % (what, n, "  ".join(("%s=%d" if isinstance(v, int) else "%s=%.3g") % (k, v)
                                                                for k, v in figures.items())))


def _avg(dev, spec, stream, F, groups=1, stride=0, linear=False, want=("mean", "peak")):
    """batch_avg on an uploaded stream: (mean rows, peak rows) as (groups, n) arrays, None where not asked for"""
    p = dev.upload(stream)
    outs = {k: dev.malloc(groups * spec.n * 4) for k in want}
    spec.batch_avg(p, F, outs.get("mean"), outs.get("peak"), groups, stride, linear)
    dev.sync()
    got = {k: dev.download(o, groups * spec.n).reshape(groups, spec.n) for k, o in outs.items()}
    for o in list(outs.values()) + [p]:
        dev.free(o)
    return got.get("mean"), got.get("peak")


def _frame_bins(dev, frames, real):
    """the bins (F, 2n) a Spectrum gives for each frame of `frames` pushed on its own"""
    F, n = frames.shape
    one = Spectrum(dev, n, real=real)
    out = np.empty((F, 2 * n), np.float32)
    for f in range(F):
        one.push_host(frames[f] if real else frames[f].view(np.float32))
        out[f] = one.get_bins()
    assert one.frames_done() == F
    one.destroy()
    return out


def _check_db(got_mean, got_peak, want_mean, want_peak, n, what, **shape):
    e_mean, o_mean = sa.masked_error(got_mean, want_mean)
    e_peak, o_peak = sa.masked_error(got_peak, want_peak)
    _say(what, n, mean_dB=e_mean, peak_dB=e_peak, left_out=max(o_mean, o_peak), **shape)
    assert max(o_mean, o_peak) <= MASK_OUT_SHARE * n
    assert e_mean <= DB_ATOL
    assert e_peak <= DB_ATOL


# ---- 1. the rule to the bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("real,n,hop", sa.BIT_SHAPES, ids=["%s-%d-%d" % ("real" if s[0] else "iq", s[1], s[2]) for s in sa.BIT_SHAPES])
def test_the_rule_to_the_bit(dev, oracle, real, n, hop):
    for F in sa.BIT_FRAMES:
        stream = sa.stream_of(real, n, hop, F)
        s = Spectrum(dev, n, hop, real=real)
        mean, peak = _avg(dev, s, stream, F, linear=True)
        s.destroy()
        want_mean, want_peak = sa.restate_linear(_frame_bins(dev, sa.group_frames(stream, real, n, hop, F), real))
        same = (int((bits_f32(mean[0]) != bits_f32(want_mean)).sum()), int((bits_f32(peak[0]) != bits_f32(want_peak)).sum()))
        _say("rule to the bit, %s" % ("real" if real else "IQ"), n, hop=hop, frames=F, mean_differ=same[0], peak_differ=same[1])
        assert same == (0, 0)
        if F == 1:
            assert np.array_equal(bits_f32(mean), bits_f32(peak))


# ---- 2. every path, every bin, in dB ------------------------------------------------------------------------------------------

EVERY = [(False,) + s for s in sa.IQ_SHAPES] + [(True,) + s for s in sa.REAL_SHAPES]


@pytest.mark.parametrize("real,n,hop,F", EVERY, ids=["%s-%d-%d-%d" % (("real" if s[0] else "iq",) + s[1:]) for s in EVERY])
def test_every_path_every_bin(dev, oracle, real, n, hop, F):
    stream, want_mean, want_peak = sa.reference_of(real, n, hop, F)
    s = Spectrum(dev, n, hop, real=real)
    mean, peak = _avg(dev, s, stream, F)
    s.destroy()
    _check_db(mean, peak, want_mean, want_peak, n, "every bin, %s" % ("real" if real else "IQ"), hop=hop, frames=F)


def test_one_output_alone_is_the_same_row(dev, oracle):
    real, n, hop, F = False, 512, 128, 70
    stream = sa.reference_of(real, n, hop, F)[0]
    s = Spectrum(dev, n, hop)
    mean, peak = _avg(dev, s, stream, F)
    only_mean = _avg(dev, s, stream, F, want=("mean",))[0]
    only_peak = _avg(dev, s, stream, F, want=("peak",))[1]
    s.destroy()
    assert np.array_equal(bits_f32(only_mean), bits_f32(mean)) and np.array_equal(bits_f32(only_peak), bits_f32(peak))


# ---- 3. groups ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("real,n,hop,F,groups,stride", sa.GROUP_SHAPES,
                         ids=["%s-%d-%d-%d-%d" % (("real" if s[0] else "iq",) + s[1:5]) for s in sa.GROUP_SHAPES])
def test_groups(dev, oracle, real, n, hop, F, groups, stride):
    """every group against the reference of its own frames; on the single-workgroup sizes to the bit as well; and one
    call with G groups gives the bits of G calls with one group each"""
    stream, want_mean, want_peak = sa.reference_of(real, n, hop, F, groups, stride)
    s = Spectrum(dev, n, hop, real=real)
    mean, peak = _avg(dev, s, stream, F, groups, stride)
    _check_db(mean, peak, want_mean, want_peak, n, "groups, %s" % ("real" if real else "IQ"), hop=hop, frames=F, groups=groups)
    lin_mean, lin_peak = _avg(dev, s, stream, F, groups, stride, linear=True)
    if n <= 8192:
        differ = 0
        for g in range(groups):
            wm, wp = sa.restate_linear(_frame_bins(dev, sa.group_frames(stream, real, n, hop, F, g, stride), real))
            differ += int((bits_f32(lin_mean[g]) != bits_f32(wm)).sum()) + int((bits_f32(lin_peak[g]) != bits_f32(wp)).sum())
        _say("groups to the bit", n, groups=groups, differ=differ)
        assert differ == 0
    # G calls with one group each: dB and linear
    ch = 1 if real else 2
    p = dev.upload(stream)
    out = dev.malloc(4 * groups * n * 4)
    for g in range(groups):
        at = p + 4 * ch * g * stride
        s.batch_avg(at, F, out + 4 * n * g, out + 4 * n * (groups + g))
        s.batch_avg(at, F, out + 4 * n * (2 * groups + g), out + 4 * n * (3 * groups + g), linear=True)
    dev.sync()
    single = dev.download(out, 4 * groups * n).reshape(4, groups, n)
    dev.free(out)
    dev.free(p)
    s.destroy()
    for a, b in zip(single, (mean, peak, lin_mean, lin_peak)):
        assert np.array_equal(bits_f32(a), bits_f32(b))


def test_a_cut_between_chunks_leaves_no_trace(dev, oracle):
    """65536 points, 259 frames: the scratch area holds 127 frames and the carry, so the call goes in three chunks, the
    first two with four frames per pass-1 workgroup.  The rule restated on each frame's bins (a second Spectrum, one
    frame per push) gives the same bits: sum and peak cross the cuts in the carry buffer unchanged."""
    real, n, hop, F = False, 65536, 1024, 259
    stream = sa.reference_of(real, n, hop, F)[0]
    s = Spectrum(dev, n, hop)
    mean, peak = _avg(dev, s, stream, F, linear=True)
    s.destroy()
    wm, wp = sa.restate_linear(_frame_bins(dev, sa.group_frames(stream, real, n, hop, F), real))
    differ = (int((bits_f32(mean[0]) != bits_f32(wm)).sum()), int((bits_f32(peak[0]) != bits_f32(wp)).sum()))
    _say("three chunks to the bit", n, frames=F, mean_differ=differ[0], peak_differ=differ[1])
    assert differ == (0, 0)


# ---- 4. the burst -----------------------------------------------------------------------------------------------------------------

def test_the_burst_shows_in_the_peak_row(dev, oracle):
    n, F, col = sa.BURST_N, sa.BURST_F, sa.BURST_COLUMN
    stream = sa.burst_stream()
    frames = sa.group_frames(stream, False, n, n, F)
    want_rows = oracle.spectrum_np(frames)[0]
    s = Spectrum(dev, n)
    mean, peak = _avg(dev, s, stream, F)
    p = dev.upload(stream)
    out = dev.malloc(F * n * 4)
    s.batch_db(p, F, out)
    dev.sync()
    rows = dev.download(out, F * n).reshape(F, n)
    dev.free(out)
    dev.free(p)
    s.destroy()
    _say("burst", n, frame3_dB=float(want_rows[sa.BURST_AT, col]), peak_dB=float(peak[0, col]), mean_dB=float(mean[0, col]),
         last_row_dB=float(rows[F - 1, col]))
    assert int(np.argmax(peak[0])) == col
    assert abs(float(peak[0, col]) - want_rows[sa.BURST_AT, col]) <= DB_ATOL
    assert abs((float(peak[0, col]) - float(mean[0, col])) - 10.0 * np.log10(8.0)) <= 0.05
    assert float(rows[F - 1, col]) < float(peak[0, col]) - 40.0


# ---- 5. a tuner's audio -----------------------------------------------------------------------------------------------------------

FS, CHAN_RATE, AUDIO_RATE, K2, NRX = 2_400_000, 240_000, 48_000, 1024, 64
AUDIO_N, AUDIO_HOP = 256, 128


def _rx_ifs():
    return [(c - NRX // 2) * 30_000 + 99 for c in range(NRX)]


def _audio_tuner(dev, stream):
    t = Tuner(dev, FS, NRX, K2 * 50, capi.WR_NCO_ROTATE)
    chans = [t.add_receiver(f, 100_000, CHAN_RATE, capi.WR_FM, 8_000, AUDIO_RATE) for f in _rx_ifs()]
    t.streaming(stream)
    return t, chans


def _audio_avg(dev, t, spec, a, stride, slots, F):
    out = dev.malloc(2 * slots * spec.n * 4)
    spec.batch_avg(a, F, out, out + slots * spec.n * 4, slots, stride)
    dev.sync()
    rows = dev.download(out, 2 * slots * spec.n).reshape(2, slots, spec.n)
    dev.free(out)
    return rows


def test_averaged_audio_spectra_of_a_tuner(dev, oracle):
    """64 receivers, one block of 1024 audio frames: the averaged 256-point audio spectrum (hop 128: 7 frames) of every
    receiver from one call on wr_tuner_audio_dev's rows, each slot in use against the reference of that slot's fetched
    audio.  With streaming on and the launch open the call closes the launch and gives the same bits."""
    F = (K2 - AUDIO_N) // AUDIO_HOP + 1
    iq = synth.fm_stream(K2 * 50, FS, _rx_ifs()[3::16], amp=0.1, fm_base=700.0, fm_step=900.0, beta=2.0)
    x = dev.upload(iq)
    spec = Spectrum(dev, AUDIO_N, AUDIO_HOP, real=True)

    t, chans = _audio_tuner(dev, False)
    t.submit_device(x, K2 * 50)
    a, stride, frames = t.audio_dev()
    assert frames == K2 and stride >= K2
    audio = t.fetch_audio_all()
    rows = _audio_avg(dev, t, spec, a, stride, audio.shape[0], F)
    worst = 0.0
    for ch in chans:
        slot = t.slot(ch)
        assert float(np.abs(audio[slot]).max()) > 0.0
        want_mean, want_peak = sa.reference_db(sa.group_frames(audio[slot], True, AUDIO_N, AUDIO_HOP, F))
        worst = max(worst, sa.masked_error(rows[0, slot], want_mean)[0], sa.masked_error(rows[1, slot], want_peak)[0])
    _say("tuner audio, 64 receivers", AUDIO_N, frames=F, dB=worst)
    assert worst <= DB_ATOL
    used = [t.slot(ch) for ch in chans]
    assert t.stream_info()[0] is False
    t.submit_device(x, K2 * 50)                         # a second block, for the streaming twin below
    a, stride, frames = t.audio_dev()
    rows2 = _audio_avg(dev, t, spec, a, stride, audio.shape[0], F)
    t.destroy()

    t, chans = _audio_tuner(dev, True)
    t.submit_device(x, K2 * 50)
    assert t.stream_info()[0] is True
    a, stride, frames = t.audio_dev()                   # (reading the audio closes the launch ...)
    t.submit_device(x, K2 * 50)                         # (... and the next block opens another)
    assert t.stream_info()[0] is True
    one = dev.malloc(spec.n * 4)
    spec.batch_avg(a, F, one)                           # a call on the device while the launch is open: closes it first
    assert t.stream_info()[0] is False
    dev.sync()
    dev.free(one)
    a, stride, frames = t.audio_dev()
    srows2 = _audio_avg(dev, t, spec, a, stride, audio.shape[0], F)
    assert [t.slot(ch) for ch in chans] == used
    assert np.array_equal(bits_f32(srows2[:, used]), bits_f32(rows2[:, used]))
    t.destroy()
    spec.destroy()
    dev.free(x)


# ---- 6. rows_waterfall ------------------------------------------------------------------------------------------------------------

def test_rows_waterfall_is_its_restatement(dev, oracle):
    """mean and peak rows of five groups and of a sixth of all-zero frames (-inf dB): exact, the palette included, at
    widths n, n / 2 and 1, hold 0 and 1.  (512 points of the flat input lie near -39 dB a bin: inside the palette's -50
    to -25 dB, which the test asserts.)"""
    n, hop, F, groups = 512, 128, 6, 5
    stride = sa.span(n, hop, F)
    stream = np.array(sa.stream_of(False, n, hop, F, groups + 1, stride))
    stream[2 * groups * stride:] = 0.0
    s = Spectrum(dev, n, hop)
    p = dev.upload(stream)
    nrows = 2 * (groups + 1)
    db = dev.malloc(nrows * n * 4)
    s.batch_avg(p, F, db, db + (groups + 1) * n * 4, groups + 1, stride)
    dev.sync()
    rows = dev.download(db, nrows * n).reshape(nrows, n)
    assert np.all(np.isneginf(rows[groups])) and np.all(np.isneginf(rows[2 * groups + 1]))
    inside = 0.0
    for width in (n, n // 2, 1):
        for hold in (0, 1):
            odb, opal = dev.malloc(nrows * width * 4), dev.malloc(max(4, nrows * width))
            s.rows_waterfall(db, nrows, width, hold, odb, opal)
            dev.sync()
            gdb = dev.download(odb, nrows * width).reshape(nrows, width)
            gpal = dev.download(opal, nrows * width, np.uint8).reshape(nrows, width)
            wdb, wpal = sa.rows_waterfall(rows, width, hold)
            assert np.array_equal(bits_f32(gdb), bits_f32(wdb)), (width, hold)
            assert np.array_equal(gpal, wpal), (width, hold)
            assert np.all(gdb[groups] == -10000.0) and np.all(gpal[groups] == 0)
            inside = max(inside, float(((wpal > 0) & (wpal < 255)).mean()))
            # either output alone
            s.rows_waterfall(db, nrows, width, hold, odb, None)
            s.rows_waterfall(db, nrows, width, hold, None, opal)
            dev.sync()
            assert np.array_equal(bits_f32(dev.download(odb, nrows * width)), bits_f32(wdb.ravel()))
            dev.free(odb)
            dev.free(opal)
    _say("rows_waterfall", n, rows=nrows, inside_palette=inside)
    assert inside >= 0.5                                  # (or the palette check would be vacuous)
    # batch_db's rows serve as well
    bdb = dev.malloc(F * n * 4)
    s.batch_db(p, F, bdb)
    o = dev.malloc(F * 8 * 4)
    s.rows_waterfall(bdb, F, 8, 1, o, None)
    dev.sync()
    assert np.array_equal(bits_f32(dev.download(o, F * 8).reshape(F, 8)),
                          bits_f32(sa.rows_waterfall(dev.download(bdb, F * n).reshape(F, n), 8, 1)[0]))
    for q in (db, p, bdb, o):
        dev.free(q)
    s.destroy()


# ---- 7. the spectrum's own state ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("real,n,hop,F", [(False, 512, 128, 9), (False, 32768, 8192, 6), (True, 65536, 4096, 5)])
def test_the_spectrum_s_own_frames_are_left_alone(dev, oracle, real, n, hop, F):
    """frames_done, get_bins and get_db after a push are the same before and after a batch_avg on other data -- on the
    two-pass sizes a batch_avg of F frames regrows the work area the push used"""
    ch = 1 if real else 2
    pushed = sa.stream_of(real, n, hop, 2, 1, 1)
    other = sa.stream_of(real, n, hop, F)
    s = Spectrum(dev, n, hop, real=real)
    s.push_host(pushed)
    before = (s.frames_done(), s.get_bins(), s.get_db())
    assert before[0] == 2 and pushed.size == ch * (n + hop)
    _avg(dev, s, other, F)
    after = (s.frames_done(), s.get_bins(), s.get_db())
    assert after[0] == before[0]
    assert np.array_equal(bits_f32(after[1]), bits_f32(before[1])) and np.array_equal(bits_f32(after[2]), bits_f32(before[2]))
    s.push_host(other[: ch * hop])                        # ... and the next push completes the next frame as ever
    assert s.frames_done() == 3
    s.destroy()


# ---- 8. argument errors -------------------------------------------------------------------------------------------------------------

def test_argument_errors(dev, oracle):
    lib = dev.lib
    n = 64
    s = Spectrum(dev, n, 16)
    p = dev.upload(np.zeros(2 * 4 * n, np.float32))
    out = dev.malloc(4 * n * 4)
    vp = C.c_void_p

    def avg(spec, src, F, G, stride, mean, peak):
        return lib.wr_spectrum_batch_avg(spec, vp(src) if src else None, F, G, stride, 0, vp(mean) if mean else None,
                                         vp(peak) if peak else None)

    for call in (lambda: avg(None, p, 1, 1, 0, out, None), lambda: avg(s.h, None, 1, 1, 0, out, None),
                 lambda: avg(s.h, p, 1, 1, 0, None, None), lambda: avg(s.h, p, 0, 1, 0, out, None),
                 lambda: avg(s.h, p, 1, 2, n - 1, out, None)):
        assert call() == capi.WR_ERR_ARG
        assert b"wr_spectrum_batch_avg" in lib.wr_last_error()
    # no groups: nothing written
    marker = np.full(n, 7.0, np.float32)
    lib.wr_dev_upload(dev.h, vp(out), capi.ptr(marker), marker.nbytes)
    assert avg(s.h, p, 1, 0, 0, out, out) == capi.WR_OK
    dev.sync()
    assert np.array_equal(dev.download(out, n), marker)
    # one group: any stride
    assert avg(s.h, p, 2, 1, 0, out, None) == capi.WR_OK
    assert avg(s.h, p, 1, 2, n, out, None) == capi.WR_OK
    dev.sync()

    def rows(spec, src, nrows, width, a, b):
        return lib.wr_spectrum_rows_waterfall(spec, vp(src) if src else None, nrows, width, 0, vp(a) if a else None, vp(b) if b else None)

    for call in (lambda: rows(None, out, 1, 8, out, None), lambda: rows(s.h, None, 1, 8, out, None),
                 lambda: rows(s.h, out, 1, 8, None, None), lambda: rows(s.h, out, 1, 0, p, None),
                 lambda: rows(s.h, out, 1, 2 * n, p, None), lambda: rows(s.h, out, 1, 24, p, None)):
        assert call() == capi.WR_ERR_ARG
        assert b"wr_spectrum_rows_waterfall" in lib.wr_last_error()
    assert rows(s.h, out, 1, 8, p, None) == capi.WR_OK
    dev.sync()
    dev.free(p)
    dev.free(out)
    s.destroy()
