/*
 * wr_levels.hip -- signal levels of the columns of a [rows][S] array of IQ frames (a tuner's channel IQ: one column per
 * channel slot; S = 1: a plain block): per column the mean and the peak of e = i*i + q*q over the block's frames and,
 * with squelch thresholds, how many audio frames the audio path's gate (audio_out, wr_kernels.hip) mutes.
 *
 * THE SUM has one order of additions, a function of the frame count alone -- not of the device, the grid or S:
 *   frames are added oldest first in runs of 16      r_j = e_16j + e_16j+1 + ...
 *   run sums are added in order in groups of 16 runs c_h = r_16h + r_16h+1 + ...        (256 frames)
 *   group sums are added in order                    sum = c_0 + c_1 + ...
 * the last run and the last group are simply shorter, and every partial starts FROM its first term (not 0.0f + term;
 * e is never -0 -- squares and their sum are +0 or above -- so the two would agree anyway).  No float atomics: their
 * result depends on who arrives first.  The group sums go to memory with plain stores and a lane per column adds them.
 *
 * Mapping (k_levels_part): a lane is a column, a wave is one RUN -- its 16 row loads (8 B per lane, 512 B per wave and
 * row, rows S * 8 bytes apart) are issued before the first is used -- and a workgroup of 16 waves is one GROUP of one
 * lane group: grid = (groups of 256 rows) x (lane groups), 160 workgroups / 2560 waves at 256 slots x 10 000 rows.
 * The run sums and maxima meet in LDS, wave 0 adds them in order.  k_levels_sum: a lane per column over the groups.
 */
#include "wr_internal.h"

/* (LV_*, the grids, the LDS and the work area's layout -- wrp_levels_plan -- are wr_plan.h's) */

/* SQ: count the audio frames the gate mutes.  Then the workgroup keeps its 256 x 64 e values in LDS (64 KiB, dynamic)
 * and adds them again in the gate's own order: audio frame k is this workgroup's when its FIRST row k * d2 lies in the
 * group; rows of it beyond the group (d2 - 1 at most per frame that straddles the edge; nearly all when d2 > 256) are
 * read from memory again -- the neighbour workgroup has just loaded them. */
template <bool SQ>
__global__ void __launch_bounds__(LV_THREADS)
k_levels_part(const float2 *__restrict__ iq, size_t S, unsigned int cols, size_t k1, unsigned int d2, size_t k2,
              const float *__restrict__ squelch, float *__restrict__ psum, float *__restrict__ ppeak,
              unsigned int *__restrict__ pmuted)
{
	extern __shared__ float lv_tile[];                 /* SQ: [LV_ROWS][64] e */
	__shared__ float rs[LV_RUNS][WR_LANES], rp[LV_RUNS][WR_LANES];
	__shared__ unsigned int rm[LV_RUNS][WR_LANES];
	const unsigned int lane = threadIdx.x & (WR_LANES - 1u), w = threadIdx.x / WR_LANES;
	const unsigned int slot = blockIdx.y * WR_LANES + lane;
	const bool on = slot < cols;
	const size_t h = blockIdx.x, row0 = h * LV_ROWS + (size_t)w * LV_RUN;
	/* (the grid has a workgroup only where the group has a row: wave 0 always has a run) */
	const unsigned int have = row0 >= k1 ? 0u : k1 - row0 < LV_RUN ? (unsigned int)(k1 - row0) : LV_RUN;   /* wave-uniform */
	if (have && on) {
		const float2 *x = iq + row0 * S + slot;
		float2 z[LV_RUN];
#pragma unroll
		for (unsigned int i = 0; i < LV_RUN; ++i)
			z[i] = i < have ? x[(size_t)i * S] : make_float2(0.0f, 0.0f);
		float r = 0.0f, p = 0.0f;
#pragma unroll
		for (unsigned int i = 0; i < LV_RUN; ++i) {
			const float e = z[i].x * z[i].x + z[i].y * z[i].y;
			if (i == 0) {
				r = e;
				p = e;
			} else if (i < have) {
				r = r + e;
				p = fmaxf(p, e);
			}
			if (SQ && i < have)
				lv_tile[(w * LV_RUN + i) * WR_LANES + lane] = e;
		}
		rs[w][lane] = r;
		rp[w][lane] = p;
	}
	__syncthreads();
	if (SQ) {
		/* audio_out's test (wr_kernels.hip), the same expression on the same values: p from 0.0f, e added oldest first,
		 * p / (float)d2 < thr, thr > 0 */
		unsigned int muted = 0;
		const float thr = on ? squelch[slot] : 0.0f;
		const size_t lo = h * LV_ROWS, hi = lo + LV_ROWS;
		const size_t kb = (lo + d2 - 1u) / d2, ke0 = (hi + d2 - 1u) / d2, ke = ke0 < k2 ? ke0 : k2;
		if (thr > 0.0f)
			for (size_t k = kb + w; k < ke; k += LV_RUNS) {
				float p = 0.0f;
				for (unsigned int i = 0; i < d2; ++i) {
					const size_t row = k * d2 + i;
					float e;
					if (row < hi) {
						e = lv_tile[(row - lo) * WR_LANES + lane];
					} else {
						const float2 z = iq[row * S + slot];
						e = z.x * z.x + z.y * z.y;
					}
					p = p + e;
				}
				if (p / (float)d2 < thr)
					++muted;
			}
		rm[w][lane] = muted;
		__syncthreads();
	}
	if (w == 0 && on) {
		const size_t left = k1 - h * LV_ROWS;
		const unsigned int runs = left >= LV_ROWS ? LV_RUNS : (unsigned int)((left + LV_RUN - 1u) / LV_RUN);
		float c = rs[0][lane], p = rp[0][lane];
		for (unsigned int j = 1; j < runs; ++j) {
			c = c + rs[j][lane];
			p = fmaxf(p, rp[j][lane]);
		}
		psum[h * cols + slot] = c;
		ppeak[h * cols + slot] = p;
		if (SQ) {
			unsigned int m = 0;
			for (unsigned int j = 0; j < LV_RUNS; ++j)
				m += rm[j][lane];
			pmuted[h * cols + slot] = m;
		}
	}
}

/* out[0][cols] = sum / (float)k1, out[1][cols] = peak, out[2][cols] = muted (unsigned; 0 without thresholds) */
__global__ void __launch_bounds__(LV_SUM_THREADS)
k_levels_sum(const float *__restrict__ psum, const float *__restrict__ ppeak, const unsigned int *__restrict__ pmuted,
             size_t groups, unsigned int cols, size_t k1, float *__restrict__ out)
{
	const unsigned int slot = blockIdx.x * blockDim.x + threadIdx.x;
	if (slot >= cols)
		return;
	float sum = psum[slot], peak = ppeak[slot];
	unsigned int muted = pmuted ? pmuted[slot] : 0u;
	for (size_t h = 1; h < groups; ++h) {
		sum = sum + psum[h * cols + slot];
		peak = fmaxf(peak, ppeak[h * cols + slot]);
		if (pmuted)
			muted += pmuted[h * cols + slot];
	}
	out[slot] = sum / (float)k1;
	out[cols + slot] = peak;
	((unsigned int *)out)[2u * cols + slot] = muted;
}

size_t wrk_chan_levels_work(unsigned int cols, size_t k1)
{
	return wrp_levels_plan(cols, k1).work_floats;
}

hipError_t wrk_chan_levels(hipStream_t st, const float *iq, size_t S, unsigned int cols, size_t k1, unsigned int d2, size_t k2,
                           const float *squelch, float *work, const float **out)
{
	const WrLevelsPlan g = wrp_levels_plan(cols, k1);
	if (!cols || !k1 || cols > S || g.groups > 0x7fffffffu || (squelch && !d2))
		return hipErrorInvalidValue;
	float *psum = work + g.psum, *ppeak = work + g.ppeak, *res = work + g.res;
	unsigned int *pmuted = (unsigned int *)(work + g.pmuted);
	const dim3 grid((unsigned int)g.groups, g.grid_y);
	if (squelch) {
		const size_t lds = g.lds_squelch;
		/* (64 KiB of dynamic LDS, all this instance ever asks for, is above the default limit of 48) */
		static bool attr_done[WR_MAX_DEVICES];
		hipError_t e = allow_lds((const void *)k_levels_part<true>, lds, attr_done);
		if (e != hipSuccess)
			return e;
		k_levels_part<true><<<grid, LV_THREADS, lds, st>>>((const float2 *)iq, S, cols, k1, d2, k2, squelch, psum, ppeak, pmuted);
	} else {
		k_levels_part<false><<<grid, LV_THREADS, 0, st>>>((const float2 *)iq, S, cols, k1, 0, 0, nullptr, psum, ppeak, nullptr);
	}
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	k_levels_sum<<<g.sum_grid, LV_SUM_THREADS, 0, st>>>(psum, ppeak, squelch ? pmuted : nullptr, g.groups, cols, k1, res);
	*out = res;
	return hipGetLastError();
}
