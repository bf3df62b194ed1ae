/*
 * cpu_host_checks.cxx -- host-only logic of the runtime that needs no GPU: FileTuner
 * (read, (u8-128)/128 conversion, loop, end of file, raw byte access) driven through
 * DspSource::run() into a capture sink; the part arithmetic of the tuner batch; the launch plans of the
 * tuner's kernels.  Built from dspblock.cxx + filetuner.cxx and two headers only.
 */
#include <string.h>

#include <vector>

#include "blockparts.h"
#include "filetuner.h"
#include "wr_plan.h"

namespace {
class Capture : public DspBlock {
public:
	Capture() : DspBlock("cap", "Capture") {}
	std::vector<float> got;
protected:
	bool init() { return true; }
	void deinit() {}
	bool process(const vector<sample_t> &in, vector<sample_t> &) {
		got.insert(got.end(), in.begin(), in.end());
		return true;
	}
};
}

extern "C" long wr_filetuner_play(const char *path, unsigned int block_frames, unsigned int nruns, int loop,
                                  float *out, size_t cap, int *ok_runs, unsigned char *last_raw, size_t *raw_frames)
{
	FileTuner t("f");
	Capture c;
	t.setSubdevice(path);
	t.setSampleRate(2048000);
	t.setChannels(2);
	t.setBlockSize(block_frames * 2);
	t.setLoop(loop != 0);
	t.connect(&c);
	*ok_runs = 0;
	if (!t.start())
		return -1;
	for (unsigned int n = 0; n < nruns; n++)
		if (t.run())
			(*ok_runs)++;
	size_t fr = 0;
	const uint8_t *raw = t.rawU8(&fr);
	*raw_frames = fr;
	if (raw && last_raw)
		memcpy(last_raw, raw, fr * 2);
	t.stop();
	size_t n = c.got.size() < cap ? c.got.size() : cap;
	memcpy(out, c.got.data(), n * sizeof(float));
	return (long)c.got.size();
}

/* RawU8Block::rawU8Buffers() = 2 is a promise: the bytes handed out for one block stay untouched until the source starts
 * producing the block after the next (the GPU runtime lets a transfer out of them run that long).  Returns 0 when, over
 * `nruns` blocks, consecutive blocks come out of different buffers and block r's bytes are still there after run r + 1. */
extern "C" int wr_filetuner_two_buffers(const char *path, unsigned int block_frames, unsigned int nruns)
{
	FileTuner t("f");
	Capture c;
	t.setSubdevice(path);
	t.setSampleRate(2048000);
	t.setChannels(2);
	t.setBlockSize(block_frames * 2);
	t.setLoop(true);
	t.connect(&c);
	if (t.rawU8Buffers() != 2)
		return 1;
	if (!t.start())
		return 2;
	const uint8_t *prev = NULL;
	std::vector<uint8_t> prev_copy;
	int rc = 0;
	for (unsigned int n = 0; n < nruns && !rc; n++) {
		if (!t.run()) {
			rc = 3;
			break;
		}
		size_t fr = 0;
		const uint8_t *raw = t.rawU8(&fr);
		if (!raw || fr != block_frames)
			rc = 4;
		else if (prev && raw == prev)
			rc = 5;                                        /* the same buffer twice in a row */
		else if (prev && memcmp(prev, prev_copy.data(), prev_copy.size()))
			rc = 6;                                        /* the block before was overwritten */
		if (!rc) {
			prev = raw;
			prev_copy.assign(raw, raw + fr * 2);
		}
	}
	t.stop();
	return rc;
}

/* ---- in how many parts a block goes through the tuner batch (blockparts.h): the arithmetic of TunerBatch::piecesFor ---- */
extern "C" unsigned int wr_block_parts(unsigned int nframes, unsigned int pieces, unsigned long q, unsigned int min_frames)
{
	return wrhost::partsOf(nframes, pieces, q, min_frames);
}

extern "C" unsigned long wr_lcm_capped(unsigned long a, unsigned long b)
{
	return wrhost::lcmCapped(a, b);
}

/* ---- the launch geometry of the tuner's kernels (csrc/wr_plan.h): the plans as flat arrays of unsigned long long, in the
 *      order of the comment at each ---- */
extern "C" unsigned int wr_plan_post_tk(void)
{
	return POST_TK;
}

/* out[5]: gmap[0], gmap[1], ngroups, rest, kmax over `nsets`; order[ngroups]: the map read back, entry by entry */
extern "C" void wr_plan_group_map(unsigned int slots_used, unsigned long long gsel, const unsigned char *nsets,
                                  unsigned long long *out, unsigned int *order)
{
	const WrGroupMap m = wrp_group_map(slots_used, gsel);
	out[0] = m.gmap[0];
	out[1] = m.gmap[1];
	out[2] = m.ngroups;
	out[3] = m.rest;
	out[4] = wrp_kmax(m, nsets);
	for (unsigned int i = 0; i < m.ngroups; i++)
		order[i] = wrp_group_at(m, i);
}

extern "C" unsigned int wr_plan_kslow(unsigned int d1, unsigned long k1)
{
	return wrp_kslow(d1, k1);
}

extern "C" int wr_plan_post_d2_supported(unsigned int d2)
{
	return wrp_post_d2_supported(d2) ? 1 : 0;
}

extern "C" unsigned long wr_plan_post_lds_bytes(unsigned int d2, unsigned int nseg)
{
	return post_lds_bytes(d2, nseg);
}

extern "C" unsigned long wr_plan_stream_lds_bytes(unsigned int d2, unsigned int nset, unsigned int nseg)
{
	return stream_lds_bytes(d2, nset, nseg);
}

extern "C" int wr_plan_stream_nseg_supported(unsigned int d2, unsigned int nseg)
{
	return stream_nseg_supported(d2, nseg) ? 1 : 0;
}

/* out[4]: ok, ng, ts, lds */
extern "C" void wr_plan_stream(unsigned int d2, unsigned int groups, unsigned int kmax, int one_filter, unsigned int nseg,
                               unsigned long long *out)
{
	const WrStreamPlan p = wrp_stream_plan(d2, groups, kmax, one_filter != 0, nseg);
	out[0] = p.ok;
	out[1] = p.ng;
	out[2] = p.ts;
	out[3] = p.lds;
}

/* rule 0: riding in a DDC launch, 1: on its own (`arg` = nseg); out[2]: run, ntiles */
extern "C" void wr_plan_post_tiling(int rule, unsigned int tiles, unsigned int groups, unsigned int arg, unsigned int *out)
{
	const WrPostTiling t = rule ? wrp_post_tiling_alone(tiles, groups, arg) : wrp_post_tiling_riding(tiles, groups);
	out[0] = t.run;
	out[1] = t.ntiles;
}

/* a block of k2 audio frames; out[8]: tiles, min_run, run, ntiles, drain_run, drain_ntiles, long_runs, widened */
extern "C" void wr_plan_stream_tiling(unsigned long k2, unsigned int groups, unsigned int n_post, unsigned int *out)
{
	const unsigned int tiles = wrp_post_tiles(k2);
	const WrStreamTiling t = wrp_post_tiling_stream(tiles, groups, n_post);
	out[0] = tiles;
	out[1] = t.min_run;
	out[2] = t.run;
	out[3] = t.ntiles;
	out[4] = t.drain_run;
	out[5] = t.drain_ntiles;
	out[6] = t.long_runs;
	out[7] = t.widened;
}

/* out[2]: n_ddc, n_post */
extern "C" void wr_plan_stream_roles(int per_cu, int num_cus, unsigned int *out)
{
	const WrStreamRoles r = wrp_stream_roles(per_cu, num_cus);
	out[0] = r.n_ddc;
	out[1] = r.n_post;
}

/* out[12]: ngroups, rest, ng, waves, kmax, lds, wgs_per_cu, post_wgs, kslow, n_bnd, units, wgs */
extern "C" void wr_plan_ddc(int nco, int utaps, unsigned int pd2, unsigned int slots_used, unsigned long long gsel,
                            const unsigned char *nsets, int one_filter, unsigned long k1, unsigned int d1, int num_cus,
                            unsigned long min_passes, unsigned int post_ntiles, unsigned int post_groups, unsigned long long *out)
{
	const WrDdcPlan p = wrp_ddc_plan(nco, utaps != 0, pd2, slots_used, gsel, nsets, one_filter != 0, k1, d1, num_cus, min_passes,
	                                 post_ntiles, post_groups);
	out[0] = p.map.ngroups;
	out[1] = p.map.rest;
	out[2] = p.ng;
	out[3] = p.waves;
	out[4] = p.kmax;
	out[5] = p.lds;
	out[6] = p.wgs_per_cu;
	out[7] = p.post_wgs;
	out[8] = p.kslow;
	out[9] = p.n_bnd;
	out[10] = p.units;
	out[11] = p.wgs;
}

/* out[8]: rot, two, wgs_r, post_wgs, roll_wgs, lds, wgs, rwgs */
extern "C" void wr_plan_long(int rotate, int one_filter, unsigned long k1, unsigned int groups, unsigned int len, unsigned int slots,
                             int num_cus, unsigned int ride_d2, unsigned int post_ntiles, unsigned int post_groups,
                             unsigned long long *out)
{
	const WrLongPlan p = wrp_long_plan(rotate != 0, one_filter != 0, k1, groups, len, slots, num_cus, ride_d2, post_ntiles, post_groups);
	out[0] = p.rot;
	out[1] = p.two;
	out[2] = p.wgs_r;
	out[3] = p.post_wgs;
	out[4] = p.roll_wgs;
	out[5] = p.lds;
	out[6] = p.wgs;
	out[7] = p.rwgs;
}

/* out[5]: tk, need, lds, lds_max, grid_x */
extern "C" void wr_plan_audio(unsigned long k2, unsigned int d2, unsigned int len, unsigned long long *out)
{
	const WrAudioPlan p = wrp_audio_plan(k2, d2, len);
	out[0] = p.tk;
	out[1] = p.need;
	out[2] = p.lds;
	out[3] = p.lds_max;
	out[4] = p.grid_x;
}

extern "C" unsigned int wr_plan_grid_for(unsigned long n, unsigned int block, unsigned int cap)
{
	return grid_for(n, block, cap);
}

/* ---- the spectrum launches ---- */
/* out[7]: points, n1, n2, sub, path, lds_max, real */
extern "C" void wr_plan_fft_shape(unsigned int n, unsigned int channels, unsigned long long *out)
{
	const WrFftShape s = wrp_fft_shape(n, channels);
	out[0] = s.points;
	out[1] = s.n1;
	out[2] = s.n2;
	out[3] = s.sub;
	out[4] = s.path;
	out[5] = s.lds_max;
	out[6] = s.real;
}

/* one batch of `batch` frames; out[11]: ct, rt, fpw, lds1, lds2, g1x, g1y, g2x, g2y, g3x, g3y */
extern "C" void wr_plan_fft_launch(unsigned int n, unsigned int channels, unsigned long batch, unsigned long long *out)
{
	const WrFftLaunch l = wrp_fft_launch(wrp_fft_shape(n, channels), batch);
	out[0] = l.ct;
	out[1] = l.rt;
	out[2] = l.fpw;
	out[3] = l.lds1;
	out[4] = l.lds2;
	out[5] = l.g1x;
	out[6] = l.g1y;
	out[7] = l.g2x;
	out[8] = l.g2y;
	out[9] = l.g3x;
	out[10] = l.g3y;
}

extern "C" unsigned long wr_plan_fft_work_frames(unsigned int n, unsigned long have, unsigned long want_frames)
{
	return wrp_fft_work_frames(n, have, want_frames);
}

extern "C" unsigned long wr_plan_fft_chunk(unsigned long remaining, unsigned long work_frames)
{
	return wrp_fft_chunk(remaining, work_frames);
}

extern "C" unsigned long wr_plan_fft_untangle_offset(unsigned long work_frames, unsigned int m)
{
	return wrp_fft_untangle_offset(work_frames, m);
}

extern "C" unsigned int wr_plan_fft_cols_ct(unsigned int n, unsigned int cols, int num_cus)
{
	return wrp_fft_cols_ct(n, cols, num_cus);
}

/* out[5]: FFT_THREADS, FFT_LDS_POINTS, FFT64K_P1_LONG_MIN, FFT_DB_GRID_CAP, FFT_WATERFALL_GRID_CAP */
extern "C" void wr_plan_fft_constants(unsigned int *out)
{
	out[0] = FFT_THREADS;
	out[1] = FFT_LDS_POINTS;
	out[2] = FFT64K_P1_LONG_MIN;
	out[3] = FFT_DB_GRID_CAP;
	out[4] = FFT_WATERFALL_GRID_CAP;
}

/* ---- wr_spectrum_batch_avg's plan ---- */
extern "C" size_t spec_avg_cap_bytes(void)
{
	return SPEC_AVG_BYTES;
}

/* fchunk, gchunk, carry and the scratch bytes of a call */
extern "C" void spec_avg_plan(unsigned int n, size_t F, size_t G, size_t *out4)
{
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	out4[0] = p.fchunk;
	out4[1] = p.gchunk;
	out4[2] = p.carry;
	out4[3] = wrp_spec_avg_bytes(n, p);
}

/* the call's chunks in the order the library walks them, `max` at most: rows of (g0, ng, f0, nf); returns how many there are */
extern "C" size_t spec_avg_chunks(unsigned int n, size_t F, size_t G, size_t max, size_t *rows)
{
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	WrSpecAvgChunk c;
	size_t count = 0;
	for (bool more = wrp_spec_avg_next(p, F, G, &c, true); more; more = wrp_spec_avg_next(p, F, G, &c, false)) {
		if (count < max) {
			rows[4 * count] = c.g0;
			rows[4 * count + 1] = c.ng;
			rows[4 * count + 2] = c.f0;
			rows[4 * count + 3] = c.nf;
		}
		++count;
		if (count > max)
			break;
	}
	return count;
}

/* path (WrFftPath) of a spectrum */
extern "C" int spec_avg_path(unsigned int n, unsigned int channels)
{
	return (int)wrp_fft_shape(n, channels).path;
}

/* launches of a call whose plan's work area holds what a call for its chunk reserves */
extern "C" size_t spec_avg_launches(unsigned int n, unsigned int channels, size_t F, size_t G)
{
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	return wrp_spec_avg_launches(n, channels, F, G, wrp_fft_work_frames(n, 1, p.fchunk));
}

extern "C" unsigned int spec_avg_reduce_grid(unsigned int n, size_t ng)
{
	return wrp_spec_reduce_grid(n, ng);
}

/* ---- wr_spectrum_rows_detect's plan ---- */
/* threads, bins of a tile, keys the LDS holds, the cap of a chunk's floors, what a workgroup may have of LDS */
extern "C" void detect_constants(size_t *out5)
{
	out5[0] = DETECT_THREADS;
	out5[1] = DETECT_TILE;
	out5[2] = DETECT_LDS_KEYS;
	out5[3] = DETECT_FLOOR_BYTES;
	out5[4] = DETECT_WG_LDS_MAX;
}

/* the field that breaks a limit, or NULL */
extern "C" const char *detect_rule_bad(unsigned int n, const wr_detect_rule *rule)
{
	return wrp_detect_rule_bad(n, rule);
}

/* nspans, chunk_rows, floor_bytes, keys_in_lds, lds_floor, lds_segments of a call with a valid rule */
extern "C" void detect_plan(const wr_detect_rule *rule, size_t nrows, size_t *out6)
{
	const WrDetectPlan p = wrp_detect_plan(rule, nrows);
	out6[0] = p.nspans;
	out6[1] = p.chunk_rows;
	out6[2] = p.floor_bytes;
	out6[3] = p.keys_in_lds;
	out6[4] = p.lds_floor;
	out6[5] = p.lds_segments;
}

/* the call's chunks in the order the library walks them, `max` at most: rows of (r0, nr, floor grid, segments grid); returns
 * how many there are */
extern "C" size_t detect_chunks(const wr_detect_rule *rule, size_t nrows, size_t max, size_t *rows)
{
	const WrDetectPlan p = wrp_detect_plan(rule, nrows);
	size_t r0 = 0, nr = 0, count = 0;
	for (bool more = wrp_detect_next(p, nrows, &r0, &nr, true); more; more = wrp_detect_next(p, nrows, &r0, &nr, false)) {
		if (count < max) {
			rows[4 * count] = r0;
			rows[4 * count + 1] = nr;
			rows[4 * count + 2] = wrp_detect_floor_grid(p, nr);
			rows[4 * count + 3] = wrp_detect_segments_grid(nr);
		}
		++count;
		if (count > max)
			break;
	}
	return count;
}

/* ---- the voice bank and the row kernels ---- */
/* out[9]: VOICE_THREADS, VOICE_PER, VOICE_CHUNK, VOICE_T_MIN, VOICE_T_MAX, VOICE_FILTERS, VOICE_LDS_FLOATS, then of a push of
 * `nframes` frames chunks, grid_x */
extern "C" void wr_plan_voice(unsigned long nframes, unsigned int *out)
{
	const WrVoicePlan p = wrp_voice_plan(nframes);
	out[0] = VOICE_THREADS;
	out[1] = VOICE_PER;
	out[2] = VOICE_CHUNK;
	out[3] = VOICE_T_MIN;
	out[4] = VOICE_T_MAX;
	out[5] = VOICE_FILTERS;
	out[6] = VOICE_LDS_FLOATS;
	out[7] = p.chunks;
	out[8] = p.grid_x;
}

extern "C" int wr_plan_voice_len_ok(unsigned int T)
{
	return wrp_voice_len_ok(T) ? 1 : 0;
}

/* out[6]: TN_THREADS, TN_CHUNK, TN_TABLE, then of a push chunks, nq, nr */
extern "C" void wr_plan_tones(unsigned long nframes, unsigned int window, unsigned long long *out)
{
	const WrTonesPlan p = wrp_tones_plan(nframes, window);
	out[0] = TN_THREADS;
	out[1] = TN_CHUNK;
	out[2] = TN_TABLE;
	out[3] = p.chunks;
	out[4] = p.nq;
	out[5] = p.nr;
}

/* a push of nq * W + nr frames on a row with `fill` frames in its open window; out[6]: a_lo, b_lo, oa, ob, ends, fill_after */
extern "C" void wr_plan_tones_cut(unsigned int fill, unsigned long long nq, unsigned int nr, unsigned int W, long long *out)
{
	const WrTonesCut c = wrp_tones_cut(fill, nq, nr, W);
	out[0] = c.a_lo;
	out[1] = c.b_lo;
	out[2] = c.oa;
	out[3] = c.ob;
	out[4] = (long long)c.ends;
	out[5] = c.fill_after;
}

/* out[3]: DC_SPAN, DC_THREADS, DC_RING */
extern "C" void wr_plan_dcs_constants(unsigned int *out)
{
	out[0] = DC_SPAN;
	out[1] = DC_THREADS;
	out[2] = DC_RING;
}

extern "C" int wr_plan_dcs_step_ok(unsigned long long step)
{
	return wrp_dcs_step_ok(step) ? 1 : 0;
}

/* the launches of a push of `nframes` frames at clock `first_frame`, `max` at most: rows of (g0, ph0, frames, room); returns
 * how many there are */
extern "C" size_t wr_plan_dcs_launches(unsigned long long first_frame, unsigned int step, size_t nframes, size_t max,
                                       unsigned long long *rows)
{
	WrDcsAt at = wrp_dcs_start(first_frame, step);
	size_t count = 0;
	for (size_t done = 0, n; done < nframes; done += n, at = wrp_dcs_after(at, step, n)) {
		n = wrp_dcs_take(at, step, nframes - done);
		if (count < max) {
			rows[4 * count] = at.g0;
			rows[4 * count + 1] = at.ph0;
			rows[4 * count + 2] = n;
			rows[4 * count + 3] = wrp_dcs_room(at, step);
		}
		++count;
		if (!n || count > max)
			break;
	}
	return count;
}

/* out[7]: RS_THREADS, RS_SPAN, RS_L_MAX, RS_RATIO_MAX, RS_P_MIN, RS_P_MAX, RS_TAPS_MAX */
extern "C" void wr_plan_resamp_constants(unsigned int *out)
{
	out[0] = RS_THREADS;
	out[1] = RS_SPAN;
	out[2] = RS_L_MAX;
	out[3] = RS_RATIO_MAX;
	out[4] = RS_P_MIN;
	out[5] = RS_P_MAX;
	out[6] = RS_TAPS_MAX;
}

extern "C" int wr_plan_resamp_limits_bad(unsigned int L, unsigned int M, unsigned int P)
{
	return wrp_resamp_limits_bad(L, M, P);
}

extern "C" unsigned long long wr_plan_resamp_out_frames(unsigned int L, unsigned int M, unsigned int nmod, unsigned long long nframes)
{
	return wrp_resamp_out_frames(L, M, nmod, nframes);
}

/* out[4]: n_out, j0, chunks, grid_x */
extern "C" void wr_plan_resamp(unsigned int L, unsigned int M, unsigned int nmod, unsigned long nframes, unsigned long long *out)
{
	const WrResampPlan p = wrp_resamp_plan(L, M, nmod, nframes);
	out[0] = p.n_out;
	out[1] = p.j0;
	out[2] = p.chunks;
	out[3] = p.grid_x;
}

/* chunk `chunk` of that push; out[6]: i0, base, lo, rem0, cnt, span */
extern "C" void wr_plan_resamp_chunk(unsigned int L, unsigned int M, unsigned int P, unsigned int nmod, unsigned long nframes,
                                     unsigned int chunk, long long *out)
{
	const WrResampPlan p = wrp_resamp_plan(L, M, nmod, nframes);
	const WrResampChunk c = wrp_resamp_chunk(L, M, P, nmod, p.j0, p.n_out, chunk);
	out[0] = (long long)c.i0;
	out[1] = c.base;
	out[2] = c.lo;
	out[3] = c.rem0;
	out[4] = c.cnt;
	out[5] = c.span;
}

/* out[11]: LV_ROWS, LV_THREADS, then groups, grid_y, lds_squelch, sum_grid, psum, ppeak, pmuted, res, work_floats */
extern "C" void wr_plan_levels(unsigned int cols, unsigned long k1, unsigned long long *out)
{
	const WrLevelsPlan p = wrp_levels_plan(cols, k1);
	out[0] = LV_ROWS;
	out[1] = LV_THREADS;
	out[2] = p.groups;
	out[3] = p.grid_y;
	out[4] = p.lds_squelch;
	out[5] = p.sum_grid;
	out[6] = p.psum;
	out[7] = p.ppeak;
	out[8] = p.pmuted;
	out[9] = p.res;
	out[10] = p.work_floats;
}

/* out[4]: AGC_THREADS, AGC_PER, AGC_TILE, AGC_WAVES */
extern "C" void wr_plan_agc(unsigned int *out)
{
	out[0] = AGC_THREADS;
	out[1] = AGC_PER;
	out[2] = AGC_TILE;
	out[3] = AGC_WAVES;
}

/* ---- device hand-over bookkeeping of DspBlock (no GPU involved: pointers are just tokens) ---- */
namespace {
struct Src : public DspSource {
	Src() : DspSource("s", "Src") {}
protected:
	bool init() { return true; }
	void deinit() {}
	bool process(const vector<sample_t> &, vector<sample_t> &out) {
		for (size_t n = 0; n < out.size(); n++)
			out[n] = (float)n;
		return true;
	}
};
/* pretends to compute on a device: publishes a token, fills the host vector only if asked to */
struct DevStage : public DspBlock {
	DevStage(const char *n, bool takesDevice) : DspBlock(n, "DevStage"), takes(takesDevice), hostFills(0),
	                                            sawUpstream(NULL), sawHostFrames(0) {}
	bool takes;
	int token;
	int hostFills;
	const void *sawUpstream;
	size_t sawHostFrames;
protected:
	bool init() { _outputSampleRate = inputSampleRate(); _outputChannels = inputChannels(); return true; }
	void deinit() {}
	bool acceptsDeviceInput() const { return takes; }
	bool process(const vector<sample_t> &in, vector<sample_t> &out) {
		sawUpstream = upstreamDeviceOutput();
		sawHostFrames = in.size() / 2;
		publishDeviceOutput(&token);
		const bool onHost = hostOutputNeeded();
		elideOutput(!onHost);
		if (onHost) {
			out.assign((size_t)currentOutputFrames() * 2, 1.0f);
			hostFills++;
		}
		return true;
	}
};
}

/* returns a bit mask of failed expectations (0 = all good) */
extern "C" int wr_handover_checks(void)
{
	int bad = 0;
	Src src;
	src.setSampleRate(48000);
	src.setChannels(2);
	src.setBlockSize(64);
	DevStage a("a", true), b("b", true), hostsink("h", false);
	src.connect(&a);
	a.connect(&b);
	if (!src.start())
		return -1;
	src.run();
	src.run();
	/* a is fed by the source: no device input, full host block; its only consumer takes device
	 * input, so a never fills its host output, and b sees a's token and an EMPTY host vector
	 * that still stands for 32 frames (b has no consumer: nobody needs its output on the host) */
	if (a.sawUpstream != NULL || a.sawHostFrames != 32) bad |= 1;
	if (a.hostFills != 0) bad |= 2;
	if (b.sawUpstream != (const void *)&a.token || b.sawHostFrames != 0) bad |= 4;
	if (b.hostFills != 0) bad |= 8;
	/* a host consumer joins b while running (hot-connect, quirk Q9): from then on b fills its host output */
	b.connect(&hostsink);
	src.run();
	if (b.hostFills != 1 || hostsink.sawHostFrames != 32) bad |= 16;
	if (hostsink.sawUpstream != (const void *)&b.token) bad |= 32;       /* published all the same */
	/* and a second, host-only consumer of a makes a fill its output too, while b keeps reading the token */
	DevStage tap("t", false);
	a.connect(&tap);
	src.run();
	if (a.hostFills != 1 || tap.sawHostFrames != 32 || b.sawUpstream != (const void *)&a.token) bad |= 64;
	src.stop();
	return bad;
}
