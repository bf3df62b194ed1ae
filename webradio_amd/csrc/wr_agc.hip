/*
 * wr_agc.hip -- automatic gain control of rows of audio (a tuner's audio[S][k2max]: one row per channel slot,
 * contiguous in time; a plain audio block: one row), in place.  The rule is include/webradio_amd.h's (wr_agc_rows):
 *
 *   L[m]   = min(bits(v[m]) & 0x7fffffff, 0x7f7fffff)
 *   E[m]   = max(L[m], E[m-1] - step, floor)                  integers, no wrap; E[-1] = the row's state word
 *   out[m] = v[m] * (target / float(E[m])), then * af_gain if it is not 1, then * scale if it is not 1
 *
 * E is a recurrence over time; in closed form, with C = E[-1] and U[j] = L[j] + j * step in 64 bits,
 *
 *   E[m] = max( max_{j <= m} U[j] - m * step,  C - (m + 1) * step,  floor ),
 *
 * (clamping to floor once at the end equals clamping at every step: max distributes over the subtraction), i.e. a
 * PREFIX MAXIMUM over integers -- exact, so the envelope has one value whatever order it is computed in.
 *
 * Mapping (k_agc_rows): a workgroup of 256 threads is a row, walked in tiles of 1024 frames, 4 consecutive frames per
 * thread (one 16-byte load and store where the row is 16-byte aligned).  A thread scans its own 4 keys, the waves run
 * a 64-lane inclusive prefix maximum over the threads' totals (__shfl_up, 6 steps of two dwords), the 4 wave totals
 * meet in LDS (two sets taken in turn: one barrier per tile).  Every thread derives the tile's last E -- the carry of
 * the next tile -- from the tile's maximum itself; the lane that holds the row's last frame stores the state word.
 * No division is replaced and nothing is fused: the file is compiled with -ffp-contract=off like the rest.
 */
#include "wr_internal.h"

/* (AGC_* are wr_plan.h's; the grid is the rows) */

__device__ __forceinline__ unsigned long long agc_max(unsigned long long a, unsigned long long b)
{
	return a > b ? a : b;
}

__device__ __forceinline__ long long agc_smax(long long a, long long b)
{
	return a > b ? a : b;
}

__global__ void __launch_bounds__(AGC_THREADS)
k_agc_rows(float *__restrict__ audio, size_t row_stride, size_t nframes, const WrAgcPar *__restrict__ par,
           unsigned int *__restrict__ state, float scale)
{
	__shared__ unsigned long long wt[2][AGC_WAVES];
	const size_t r = blockIdx.x;
	const WrAgcPar P = par[r];
	float *row = audio + r * row_stride;
	if (P.step > 0x80000000u) {
		/* no AGC on this row: the sink's scale alone (and not even a load where that is 1, or the row is nobody's) */
		if (P.step != WR_AGC_OFF || scale == 1.0f)
			return;
		for (size_t m = threadIdx.x; m < nframes; m += AGC_THREADS)
			row[m] = row[m] * scale;
		return;
	}
	const unsigned int lane = threadIdx.x & (WR_LANES - 1u), w = threadIdx.x / WR_LANES;
	const unsigned int j0 = threadIdx.x * AGC_PER;              /* the thread's first frame of a tile */
	const unsigned long long step = P.step;
	const long long floor_e = P.floor_bits;
	long long carry = state[r];                                 /* E of the frame before the tile's first */
	const bool wide = ((uintptr_t)row & 15u) == 0;              /* (tiles begin a multiple of 4 KiB into the row) */
	unsigned int set = 0;
	for (size_t base = 0; base < nframes; base += AGC_TILE, set ^= 1u) {
		const size_t left = nframes - base;
		const unsigned int n = left < AGC_TILE ? (unsigned int)left : AGC_TILE;     /* frames of this tile */
		float *x = row + base + j0;
		const bool whole = wide && j0 + AGC_PER <= n;
		float v[AGC_PER];
		if (whole) {
			const float4 q = *(const float4 *)x;
			v[0] = q.x;
			v[1] = q.y;
			v[2] = q.z;
			v[3] = q.w;
		} else {
#pragma unroll
			for (unsigned int i = 0; i < AGC_PER; ++i)
				v[i] = j0 + i < n ? x[i] : 0.0f;
		}
		/* the thread's own keys and their running maximum (frames beyond the tile's end count as silence: they
		 * reach only frames behind them, of which there are none) */
		unsigned long long p[AGC_PER], run = 0;
#pragma unroll
		for (unsigned int i = 0; i < AGC_PER; ++i) {
			const unsigned int a = __float_as_uint(v[i]) & 0x7fffffffu;
			const unsigned int l = a < 0x7f7fffffu ? a : 0x7f7fffffu;
			run = agc_max(run, l + (unsigned long long)(j0 + i) * step);
			p[i] = run;
		}
		/* inclusive prefix maximum of the threads' totals over the wave; keys are >= 0, so 0 is the identity */
		unsigned long long inc = run;
#pragma unroll
		for (unsigned int d = 1; d < WR_LANES; d <<= 1) {
			const unsigned long long o = __shfl_up(inc, d);
			if (lane >= d)
				inc = agc_max(inc, o);
		}
		unsigned long long before = __shfl_up(inc, 1u);         /* ... of the threads in front of this one */
		if (lane == 0)
			before = 0;
		if (lane == WR_LANES - 1u)
			wt[set][w] = inc;
		__syncthreads();
		unsigned long long tile_max = 0;
#pragma unroll
		for (unsigned int u = 0; u < AGC_WAVES; ++u) {
			const unsigned long long t = wt[set][u];
			if (u < w)
				before = agc_max(before, t);
			tile_max = agc_max(tile_max, t);
		}
		float o[AGC_PER];
#pragma unroll
		for (unsigned int i = 0; i < AGC_PER; ++i) {
			const unsigned long long back = (unsigned long long)(j0 + i) * step;
			long long e = (long long)(agc_max(before, p[i]) - back);
			e = agc_smax(e, agc_smax(carry - (long long)(back + step), floor_e));
			const float env = __uint_as_float((unsigned int)e);
			const float g = P.target / env;
			float y = v[i] * g;
			if (P.af_gain != 1.0f)
				y = y * P.af_gain;
			o[i] = (scale == 1.0f) ? y : y * scale;
			if (base + j0 + i == nframes - 1u)
				state[r] = (unsigned int)e;
		}
		if (whole) {
			*(float4 *)x = make_float4(o[0], o[1], o[2], o[3]);
		} else {
#pragma unroll
			for (unsigned int i = 0; i < AGC_PER; ++i)
				if (j0 + i < n)
					x[i] = o[i];
		}
		/* E of the tile's last frame (a whole tile's: behind a short one nothing follows) */
		carry = agc_smax(agc_smax((long long)tile_max - (long long)((AGC_TILE - 1u) * step),
		                          carry - (long long)(AGC_TILE * step)), floor_e);
	}
}

hipError_t wrk_agc_rows(hipStream_t st, float *audio, size_t row_stride, size_t nrows, size_t nframes, const WrAgcPar *par,
                        unsigned int *state, float scale)
{
	if (!nrows || !nframes)
		return hipSuccess;
	if (!audio || !par || !state || nrows > 0x7fffffffu || (nrows > 1 && row_stride < nframes))
		return hipErrorInvalidValue;
	k_agc_rows<<<(unsigned int)nrows, AGC_THREADS, 0, st>>>(audio, row_stride, nframes, par, state, scale);
	return hipGetLastError();
}
