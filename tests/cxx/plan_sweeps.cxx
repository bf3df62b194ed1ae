/*
 * plan_sweeps.cxx -- the row kernels' and the voice bank's plans (webradio_amd/csrc/wr_plan.h) swept on the CPU by a program of
 * its own: the properties tests/test_launch_plan.py holds, over more cases, for a build with the host compiler's address and
 * undefined-behaviour sanitizers (make -C tests/cxx check-plans).  No HIP, no Python.  Exit status 0: every property held.
 */
#include <stdio.h>

#include "wr_plan.h"

static unsigned long failures;

#define HOLD(cond, ...)                                                                  \
	do {                                                                                 \
		if (!(cond)) {                                                                   \
			if (failures++ < 20) {                                                       \
				fprintf(stderr, "plan_sweeps: %s does not hold: ", #cond);               \
				fprintf(stderr, __VA_ARGS__);                                            \
				fprintf(stderr, "\n");                                                   \
			}                                                                            \
		}                                                                                \
	} while (0)

/* the tone bank: ends and fill_after by walking the push window by window; the stretches lie inside the push, in order */
static void sweep_tones(unsigned int W, unsigned int fill_step, unsigned long long n_step)
{
	for (unsigned int fill = 0; fill < W; fill += fill_step)
		for (unsigned long long n = 1; n < 3ull * W; n += n_step) {
			const WrTonesPlan p = wrp_tones_plan((size_t)n, W);
			const WrTonesCut c = wrp_tones_cut(fill, p.nq, p.nr, W);
			unsigned long long ends = 0, f = fill, left = n;
			while (left) {
				const unsigned long long take = W - f < left ? W - f : left;
				left -= take;
				f += take;
				if (f == W) {
					++ends;
					f = 0;
				}
			}
			HOLD(p.nq * W + p.nr == n && p.nr < W && p.chunks == (n + TN_CHUNK - 1u) / TN_CHUNK, "W %u n %llu", W, n);
			HOLD(c.ends == ends && c.fill_after == f, "W %u fill %u n %llu", W, fill, n);
			HOLD(0 <= c.a_lo && c.a_lo <= c.b_lo && c.b_lo <= (long long)n, "W %u fill %u n %llu", W, fill, n);
			HOLD(c.oa <= c.a_lo && c.a_lo - c.oa < (long long)W && c.ob <= c.b_lo && (long long)n - c.ob <= (long long)W,
			     "W %u fill %u n %llu", W, fill, n);
			HOLD(ends ? c.b_lo - c.oa == (long long)W && c.ob == c.b_lo : c.b_lo == 0 && c.ob == -(long long)fill,
			     "W %u fill %u n %llu", W, fill, n);
		}
}

/* the DCS bank: the launches' frames sum to the push, none is empty, each stays within DC_SPAN chips, room is 510 at least,
 * and a launch begins where the clock's 128-bit product says */
static void sweep_dcs(unsigned long long first_frame, unsigned int step, size_t nframes)
{
	WrDcsAt at = wrp_dcs_start(first_frame, step);
	unsigned __int128 clock = (unsigned __int128)first_frame * step;
	size_t done = 0;
	while (done < nframes) {
		const size_t room = wrp_dcs_room(at, step), n = wrp_dcs_take(at, step, nframes - done);
		HOLD(at.g0 == (unsigned long long)(clock >> DC_CHIP_BITS) && at.ph0 == (unsigned int)(clock & ((1u << DC_CHIP_BITS) - 1u)),
		     "first %llu step %u at %zu", first_frame, step, done);
		HOLD(room >= 510u && n >= 1u && n <= room, "first %llu step %u at %zu", first_frame, step, done);
		HOLD(((at.ph0 + (unsigned long long)n * step) >> DC_CHIP_BITS) < DC_SPAN, "first %llu step %u at %zu", first_frame, step, done);
		HOLD(((at.ph0 + (unsigned long long)(room + 1u) * step) >> DC_CHIP_BITS) >= DC_SPAN, "first %llu step %u at %zu", first_frame,
		     step, done);
		if (!n)
			return;
		clock += (unsigned __int128)n * step;
		at = wrp_dcs_after(at, step, n);
		done += n;
	}
	HOLD(done == nframes, "first %llu step %u", first_frame, step);
}

/* the resampler at one clock: the chunks against the closed form, the span within RS_SPAN and within the push */
static void sweep_resamp_push(unsigned int L, unsigned int M, unsigned int P, unsigned int nmod, size_t n)
{
	const WrResampPlan p = wrp_resamp_plan(L, M, nmod, n);
	const unsigned long long j0 = ((unsigned long long)nmod * L + M - 1u) / M;
	HOLD(p.n_out == wrp_resamp_out_frames(L, M, nmod, n) && p.j0 == j0 && p.grid_x == p.chunks + 1u &&
	     p.chunks == (p.n_out + RS_THREADS - 1u) / RS_THREADS, "%u / %u clock %u n %zu", L, M, nmod, n);
	for (unsigned int i = 0; i < p.chunks; i += (p.chunks > 64u ? p.chunks / 61u : 1u)) {
		const WrResampChunk c = wrp_resamp_chunk(L, M, P, nmod, p.j0, p.n_out, i);
		const unsigned long long t = (j0 + (unsigned long long)RS_THREADS * i) * M;
		HOLD(c.i0 == (unsigned long long)RS_THREADS * i && c.base == (long long)(t / L) - (long long)nmod && c.rem0 == t % L &&
		     c.lo == c.base - (long long)(P - 1u), "%u / %u clock %u n %zu chunk %u", L, M, nmod, n, i);
		HOLD(c.cnt >= 1u && c.cnt <= RS_THREADS && c.cnt == (p.n_out - c.i0 < RS_THREADS ? p.n_out - c.i0 : RS_THREADS),
		     "%u / %u clock %u n %zu chunk %u", L, M, nmod, n, i);
		HOLD(c.span == (t + (unsigned long long)(c.cnt - 1u) * M) / L - t / L + P && c.span <= RS_SPAN && c.base >= 0 &&
		     c.lo + (long long)c.span <= (long long)n, "%u / %u clock %u n %zu chunk %u", L, M, nmod, n, i);
	}
}

static void sweep_resamp(unsigned int L, unsigned int M, unsigned int P, unsigned int clock_step)
{
	static const size_t cuts[] = {1, 1, 7, 255, 256, 257, 300, 5000, 13, (size_t)1 << 28, 1, ((size_t)1 << 28) - 1u};
	HOLD(!wrp_resamp_limits_bad(L, M, P), "%u / %u, %u taps", L, M, P);
	unsigned long long total = 0, N = 0;
	unsigned int nmod = 0;
	for (size_t k = 0; k < sizeof(cuts) / sizeof(cuts[0]); ++k) {
		total += wrp_resamp_out_frames(L, M, nmod, cuts[k]);
		sweep_resamp_push(L, M, P, nmod, cuts[k]);
		N += cuts[k];
		nmod = (unsigned int)((nmod + cuts[k]) % M);
	}
	HOLD(total == (N * L + M - 1u) / M, "%u / %u", L, M);
	for (unsigned int r = 0; r < M; r += clock_step)
		sweep_resamp_push(L, M, P, r, 3000);
}

static void sweep_levels_voice_agc(void)
{
	static const size_t k1s[] = {1, LV_ROWS - 1u, LV_ROWS, LV_ROWS + 1u, 10000, (size_t)1 << 28};
	for (size_t k = 0; k < sizeof(k1s) / sizeof(k1s[0]); ++k)
		for (unsigned int cols = 1; cols <= 4097u; cols += (cols < 130u ? 1u : 661u)) {
			const WrLevelsPlan p = wrp_levels_plan(cols, k1s[k]);
			const size_t part = p.groups * cols;
			HOLD(p.groups * LV_ROWS >= k1s[k] && (p.groups - 1u) * LV_ROWS < k1s[k], "k1 %zu", k1s[k]);
			HOLD(p.grid_y * WR_LANES >= cols && (p.grid_y - 1u) * WR_LANES < cols && p.sum_grid * LV_SUM_THREADS >= cols, "cols %u", cols);
			HOLD(p.psum == 0 && p.ppeak == part && p.pmuted == 2u * part && p.res == 3u * part && p.work_floats == p.res + 3u * cols,
			     "k1 %zu cols %u", k1s[k], cols);
		}
	for (size_t n = 1; n <= 3u * VOICE_CHUNK; ++n) {
		const WrVoicePlan v = wrp_voice_plan(n);
		HOLD(v.chunks * VOICE_CHUNK >= n && (v.chunks - 1u) * VOICE_CHUNK < n && v.grid_x == v.chunks + 1u && v.threads == VOICE_THREADS,
		     "n %zu", n);
	}
	HOLD(wrp_voice_plan((size_t)1 << 28).chunks == (1u << 28) / VOICE_CHUNK, "2^28 frames");
	HOLD(AGC_TILE == AGC_THREADS * AGC_PER && AGC_WAVES * WR_LANES == AGC_THREADS, "agc");
}

int main(void)
{
	sweep_tones(16, 1, 1);
	sweep_tones(65536, 4099, 8191);
	sweep_tones(65536, 65535, 1);
	static const unsigned int steps[] = {DC_STEP_MIN, DC_STEP_MIN + 1u, 0x0abcdef1u, DC_STEP_MAX - 1u, DC_STEP_MAX};
	static const unsigned long long firsts[] = {0, 1, 7, 12345, (1ull << 37) + 1u, (1ull << 46) + 3u, ~0ull - ((size_t)1 << 28)};
	for (size_t s = 0; s < sizeof(steps) / sizeof(steps[0]); ++s)
		for (size_t f = 0; f < sizeof(firsts) / sizeof(firsts[0]); ++f) {
			sweep_dcs(firsts[f], steps[s], 1);
			sweep_dcs(firsts[f], steps[s], 510);
			sweep_dcs(firsts[f], steps[s], 100000);
		}
	sweep_dcs(0, DC_STEP_MIN, (size_t)1 << 28);
	sweep_dcs(3, DC_STEP_MAX, (size_t)1 << 24);
	sweep_resamp(1, 8, 64, 1);
	sweep_resamp(1024, 8192, 4, 89);
	sweep_resamp(1024, 128, 16, 1);
	sweep_resamp(3, 2, 4, 1);
	sweep_resamp(441, 500, 32, 1);
	sweep_levels_voice_agc();
	if (failures) {
		fprintf(stderr, "plan_sweeps: %lu properties did not hold\n", failures);
		return 1;
	}
	printf("plan_sweeps: every property held\n");
	return 0;
}
