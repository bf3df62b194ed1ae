"""The launch plans of the tuner's kernels, of the spectrum launches, of the voice bank and of the row kernels
(webradio_amd/csrc/wr_plan.h) through tests/cxx/libwr_cpu_host_checks.so, the one road by which a test reaches them: plain
arithmetic, no GPU.  What tests/test_launch_plan.py holds to hand-worked figures, and where a GPU test that has to know which
branch of a rule a case reaches asks the rule itself."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXXT = os.path.join(ROOT, "tests", "cxx")

WR_NCO_SPLIT, WR_NCO_EXACT, WR_NCO_ROTATE = 0, 1, 2     # include/webradio_amd.h

GroupMap = namedtuple("GroupMap", "gmap0 gmap1 ngroups rest kmax order")
StreamPlan = namedtuple("StreamPlan", "ok ng ts lds")
StreamTiling = namedtuple("StreamTiling", "tiles min_run run ntiles drain_run drain_ntiles long_runs widened")
DdcPlan = namedtuple("DdcPlan", "ngroups rest ng waves kmax lds wgs_per_cu post_wgs kslow n_bnd units wgs")
LongPlan = namedtuple("LongPlan", "rot two wgs_r post_wgs roll_wgs lds wgs rwgs")
AudioPlan = namedtuple("AudioPlan", "tk need lds lds_max grid_x")
FFT_SINGLE, FFT_FOUR_STEP, FFT_REG64K = 0, 1, 2           # WrFftPath
FftShape = namedtuple("FftShape", "points n1 n2 sub path lds_max real")
FftLaunch = namedtuple("FftLaunch", "ct rt fpw lds1 lds2 grid1 grid2 grid3")
VoicePlan = namedtuple("VoicePlan", "threads per chunk t_min t_max filters lds_floats chunks grid_x")
TonesPlan = namedtuple("TonesPlan", "threads chunk table chunks nq nr")
TonesCut = namedtuple("TonesCut", "a_lo b_lo oa ob ends fill_after")
DcsLaunch = namedtuple("DcsLaunch", "g0 ph0 frames room")
ResampPlan = namedtuple("ResampPlan", "n_out j0 chunks grid_x")
ResampChunk = namedtuple("ResampChunk", "i0 base lo rem0 cnt span")
LevelsPlan = namedtuple("LevelsPlan", "rows threads groups grid_y lds_squelch sum_grid psum ppeak pmuted res work_floats")
AgcPlan = namedtuple("AgcPlan", "threads per tile waves")

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(CXXT, "libwr_cpu_host_checks.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", CXXT, "libwr_cpu_host_checks.so"])
        L = C.CDLL(path)
        u, ul, ull, i, sz = C.c_uint, C.c_ulong, C.c_ulonglong, C.c_int, C.c_size_t
        pu, pull, pb, pll, psz = C.POINTER(u), C.POINTER(ull), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong), C.POINTER(sz)
        from webradio_amd import capi
        rule = C.POINTER(capi.DetectRule)
        for name, res, args in [
            ("wr_plan_post_tk", u, []),
            ("wr_plan_group_map", None, [u, ull, pb, pull, pu]),
            ("wr_plan_kslow", u, [u, ul]),
            ("wr_plan_post_d2_supported", i, [u]),
            ("wr_plan_post_lds_bytes", ul, [u, u]),
            ("wr_plan_stream_lds_bytes", ul, [u, u, u]),
            ("wr_plan_stream_nseg_supported", i, [u, u]),
            ("wr_plan_stream", None, [u, u, u, i, u, pull]),
            ("wr_plan_post_tiling", None, [i, u, u, u, pu]),
            ("wr_plan_stream_tiling", None, [ul, u, u, pu]),
            ("wr_plan_stream_roles", None, [i, i, pu]),
            ("wr_plan_ddc", None, [i, i, u, u, ull, pb, i, ul, u, i, ul, u, u, pull]),
            ("wr_plan_long", None, [i, i, ul, u, u, u, i, u, u, u, pull]),
            ("wr_plan_audio", None, [ul, u, u, pull]),
            ("wr_plan_grid_for", u, [ul, u, u]),
            ("wr_plan_fft_shape", None, [u, u, pull]),
            ("wr_plan_fft_launch", None, [u, u, ul, pull]),
            ("wr_plan_fft_work_frames", ul, [u, ul, ul]),
            ("wr_plan_fft_chunk", ul, [ul, ul]),
            ("wr_plan_fft_untangle_offset", ul, [ul, u]),
            ("wr_plan_fft_cols_ct", u, [u, u, i]),
            ("wr_plan_fft_constants", None, [pu]),
            ("spec_avg_cap_bytes", sz, []),
            ("spec_avg_plan", None, [u, sz, sz, psz]),
            ("spec_avg_chunks", sz, [u, sz, sz, sz, psz]),
            ("spec_avg_path", i, [u, u]),
            ("spec_avg_launches", sz, [u, u, sz, sz]),
            ("spec_avg_reduce_grid", u, [u, sz]),
            ("detect_constants", None, [psz]),
            ("detect_rule_bad", C.c_char_p, [u, rule]),
            ("detect_plan", None, [rule, sz, psz]),
            ("detect_chunks", sz, [rule, sz, sz, psz]),
            ("wr_plan_voice", None, [ul, pu]),
            ("wr_plan_voice_len_ok", i, [u]),
            ("wr_plan_tones", None, [ul, u, pull]),
            ("wr_plan_tones_cut", None, [u, ull, u, u, pll]),
            ("wr_plan_dcs_constants", None, [pu]),
            ("wr_plan_dcs_step_ok", i, [ull]),
            ("wr_plan_dcs_launches", sz, [ull, u, sz, sz, pull]),
            ("wr_plan_resamp_constants", None, [pu]),
            ("wr_plan_resamp_limits_bad", i, [u, u, u]),
            ("wr_plan_resamp_out_frames", ull, [u, u, u, ull]),
            ("wr_plan_resamp", None, [u, u, u, ul, pull]),
            ("wr_plan_resamp_chunk", None, [u, u, u, u, ul, u, pll]),
            ("wr_plan_levels", None, [u, ul, pull]),
            ("wr_plan_agc", None, [pu]),
        ]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def _nsets(nsets):
    return (C.c_ubyte * 64)(*(list(nsets) + [1] * (64 - len(nsets))))


def post_tk():
    return lib().wr_plan_post_tk()


def group_map(groups, gsel=0, nsets=()):
    out, order = (C.c_ulonglong * 5)(), (C.c_uint * 16)()
    lib().wr_plan_group_map(64 * groups, gsel, _nsets(nsets), out, order)
    return GroupMap(out[0], out[1], out[2], out[3], out[4], list(order[:out[2]]))


def stream_plan(d2, groups, kmax, one_filter, nseg):
    out = (C.c_ulonglong * 4)()
    lib().wr_plan_stream(d2, groups, kmax, int(one_filter), nseg, out)
    return StreamPlan(bool(out[0]), *out[1:])


def post_tiling_riding(tiles, groups):
    out = (C.c_uint * 2)()
    lib().wr_plan_post_tiling(0, tiles, groups, 0, out)
    return tuple(out)


def post_tiling_alone(tiles, groups, nseg=1):
    out = (C.c_uint * 2)()
    lib().wr_plan_post_tiling(1, tiles, groups, nseg, out)
    return tuple(out)


def stream_tiling(k2, groups, n_post):
    out = (C.c_uint * 8)()
    lib().wr_plan_stream_tiling(k2, groups, n_post, out)
    return StreamTiling(*out[:6], bool(out[6]), out[7])


def stream_roles(per_cu, num_cus):
    out = (C.c_uint * 2)()
    lib().wr_plan_stream_roles(per_cu, num_cus, out)
    return tuple(out)


def ddc_plan(nco, utaps, pd2, groups, k1, d1, num_cus, one_filter=True, min_passes=4, gsel=0, nsets=(), post_ntiles=0,
             post_groups=0):
    out = (C.c_ulonglong * 12)()
    lib().wr_plan_ddc(nco, int(utaps), pd2, 64 * groups, gsel, _nsets(nsets), int(one_filter), k1, d1, num_cus, min_passes,
                      post_ntiles, post_groups, out)
    return DdcPlan(*out)


def long_plan(rotate, one_filter, k1, groups, length, slots, num_cus, ride_d2=0, post_ntiles=0, post_groups=0):
    out = (C.c_ulonglong * 8)()
    lib().wr_plan_long(int(rotate), int(one_filter), k1, groups, length, slots, num_cus, ride_d2, post_ntiles, post_groups, out)
    return LongPlan(bool(out[0]), bool(out[1]), *out[2:])


def audio_plan(k2, d2, length):
    out = (C.c_ulonglong * 5)()
    lib().wr_plan_audio(k2, d2, length, out)
    return AudioPlan(*out)


def fft_shape(n, real=False):
    out = (C.c_ulonglong * 7)()
    lib().wr_plan_fft_shape(n, 1 if real else 2, out)
    return FftShape(*out[:6], bool(out[6]))


def fft_launch(n, batch, real=False):
    """one batch; the grids as (x, y), (0, 0): no such launch"""
    o = (C.c_ulonglong * 11)()
    lib().wr_plan_fft_launch(n, 1 if real else 2, batch, o)
    return FftLaunch(*o[:5], (o[5], o[6]), (o[7], o[8]), (o[9], o[10]))


def fft_work_frames(n, have, want_frames):
    return lib().wr_plan_fft_work_frames(n, have, want_frames)


def fft_chunks(n, frames, have=1):
    """the batches a call of `frames` frames runs as, after the work area has grown for it"""
    work, left, got = fft_work_frames(n, have, frames), frames, []
    while left:
        got.append(lib().wr_plan_fft_chunk(left, work))
        left -= got[-1]
    return got


def fft_cols_ct(n, cols, num_cus):
    return lib().wr_plan_fft_cols_ct(n, cols, num_cus)


def fft_constants():
    out = (C.c_uint * 5)()
    lib().wr_plan_fft_constants(out)
    return dict(zip("threads lds_points p1_long_min db_grid_cap waterfall_grid_cap".split(), out))


# ---- the voice bank and the row kernels ------------------------------------------------------------------------------------

def voice_plan(nframes=1):
    """the constants, and chunks and grid_x of a push of `nframes` frames"""
    out = (C.c_uint * 9)()
    lib().wr_plan_voice(nframes, out)
    return VoicePlan(*out)


def tones_plan(nframes, window):
    out = (C.c_ulonglong * 6)()
    lib().wr_plan_tones(nframes, window, out)
    return TonesPlan(*out)


def tones_cut(fill, n, W):
    """a push of n frames on a row with `fill` frames in its open window of W"""
    out = (C.c_longlong * 6)()
    lib().wr_plan_tones_cut(fill, n // W, n % W, W, out)
    return TonesCut(*out)


def dcs_constants():
    out = (C.c_uint * 3)()
    lib().wr_plan_dcs_constants(out)
    return dict(zip("span threads ring".split(), out))


def dcs_launches(first_frame, step, nframes, most=1 << 20):
    rows = (C.c_ulonglong * (4 * most))()
    count = lib().wr_plan_dcs_launches(first_frame, step, nframes, most, rows)
    assert count <= most, "more launches than the test walks"
    return [DcsLaunch(*rows[4 * k: 4 * k + 4]) for k in range(count)]


def resamp_constants():
    out = (C.c_uint * 7)()
    lib().wr_plan_resamp_constants(out)
    return dict(zip("threads span l_max ratio_max p_min p_max taps_max".split(), out))


def resamp_out_frames(L, M, nmod, nframes):
    return lib().wr_plan_resamp_out_frames(L, M, nmod, nframes)


def resamp_plan(L, M, nmod, nframes):
    out = (C.c_ulonglong * 4)()
    lib().wr_plan_resamp(L, M, nmod, nframes, out)
    return ResampPlan(*out)


def resamp_chunk(L, M, P, nmod, nframes, chunk):
    out = (C.c_longlong * 6)()
    lib().wr_plan_resamp_chunk(L, M, P, nmod, nframes, chunk, out)
    return ResampChunk(*out)


def levels_plan(cols, k1):
    out = (C.c_ulonglong * 11)()
    lib().wr_plan_levels(cols, k1, out)
    return LevelsPlan(*out)


def agc_plan():
    out = (C.c_uint * 4)()
    lib().wr_plan_agc(out)
    return AgcPlan(*out)
