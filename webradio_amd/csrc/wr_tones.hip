/*
 * wr_tones.hip -- a bank of up to 64 tone correlators over rows of audio (a tuner's audio[S][k2max]: one row per channel
 * slot; a plain block of rows), integrated over windows of W frames that run on from push to push.  The rule is
 * include/webradio_amd.h's (wr_tones_push_rows); for frame j of a window, audio value v, tone t:
 *
 *   w    = min(max(v', -64), 64) * 2^24          v' = 0 for an inf or a NaN; |w| <= 2^30
 *   p    = (uint32)(j * step_t),  i = p >> 20,  s = T12[i],  c = T12[(i + 1024) & 4095]
 *   I_t += (int64)rint(w * c),  Q_t += (int64)rint(w * s),  E += ((int64)rint(w))^2 >> 14
 *
 * Every sum is one of INTEGERS, so a window has one result whatever the grid, the cut into pushes and the order:
 * the partial sums below may meet in any order, integer atomics included.
 *
 * What a push of n frames holds for a row with f frames in its open window: `ends` = (f + n) / W window ends.  Only two
 * stretches of its frames are summed --
 *   A: the LAST window that ends in the push (from frame max(ends * W - f - W, 0) of the push; where that window began in
 *      an earlier push, ends = 1 and f > 0, k_tones_latch joins the carried sums to it)
 *   B: the open window behind it (all of the push when ends = 0)
 * -- frames of earlier windows that lie wholly inside the push are only counted.
 *
 * Mapping (k_tones_part): a LANE IS A TONE.  A workgroup of 4 waves is TN_CHUNK = 512 frames of one row: the 4096-entry
 * table (16 KiB) and the chunk's w (2 KiB; a thread converts two frames and adds their E terms) sit in LDS; wave u walks
 * frames [128 u, 128 u + 128) of the chunk with w wave-uniform (one broadcast LDS read), I and Q in 64-bit registers per
 * lane and p advanced by step -- two LDS gathers, two products, two rint and two 64-bit additions per tone and frame.  The
 * waves' sums meet in LDS, and thread i adds word i of the workgroup's [A, B][tone][I, Q] to the row's `part` with one
 * 64-bit integer atomicAdd: 256 contiguous 8-byte words per workgroup.  Workgroups whose chunk lies in front of A return
 * at once.  k_tones_latch, a workgroup of 64 lanes per row, latches, carries, counts and leaves `part` zero again.
 */
#include "wr_internal.h"
#include "wr_rows.h"

/* (TN_*, the launch figures and the cut of a push -- wrp_tones_cut -- are wr_plan.h's) */

__global__ void __launch_bounds__(TN_THREADS)
k_tones_part(const float *__restrict__ audio, size_t row_stride, size_t nframes, unsigned long long nq, unsigned int nr,
             WrTonesRow *__restrict__ rows, const float *__restrict__ t12, const unsigned int *__restrict__ steps,
             unsigned int ntones, unsigned int W)
{
	__shared__ float tab[TN_TABLE];
	__shared__ float wv[TN_CHUNK];
	__shared__ long long red[TN_WAVES][2u * WR_LANES * 2u];      /* per wave [A, B][tone][I, Q] */
	__shared__ long long red_e[TN_WAVES][2];
	const unsigned int tid = threadIdx.x, lane = tid & (WR_LANES - 1u), u = tid / WR_LANES;
	WrTonesRow *R = rows + blockIdx.y;
	const WrTonesCut cut = wrp_tones_cut(R->fill, nq, nr, W);
	const long long k0 = (long long)blockIdx.x * TN_CHUNK;
	const long long k1 = k0 + TN_CHUNK < (long long)nframes ? k0 + TN_CHUNK : (long long)nframes;
	if (k1 <= cut.a_lo)                                          /* whole windows in front of the last: only counted */
		return;
	for (unsigned int i = tid; i < TN_TABLE / 4u; i += TN_THREADS)
		((float4 *)tab)[i] = ((const float4 *)t12)[i];
	const float *row = audio + (size_t)blockIdx.y * row_stride;
	long long e_a = 0, e_b = 0;
	for (unsigned int i = tid; i < TN_CHUNK; i += TN_THREADS) {
		const long long k = k0 + i;
		if (k >= k1)
			break;
		const float w = row_fixed24(row[k]);
		wv[i] = w;
		const long long qv = (long long)(int)rintf(w);
		const long long e = (qv * qv) >> 14;
		if (k >= cut.b_lo)
			e_b += e;
		else if (k >= cut.a_lo)
			e_a += e;
	}
	__syncthreads();
	/* the wave's frames, stretch A then stretch B */
	const unsigned int step = steps[lane];                        /* (0 beyond the bank's tones: those lanes' sums are dropped) */
	const long long lo = k0 + (long long)(u * TN_RUN), hi = lo + TN_RUN < k1 ? lo + TN_RUN : k1;
#pragma unroll
	for (unsigned int seg = 0; seg < 2u; ++seg) {
		const long long s_lo = seg ? cut.b_lo : cut.a_lo, s_hi = seg ? (long long)nframes : cut.b_lo;
		const long long origin = seg ? cut.ob : cut.oa;
		const long long from = lo > s_lo ? lo : s_lo, to = hi < s_hi ? hi : s_hi;
		long long I = 0, Q = 0;
		if (from < to) {
			unsigned int p = (unsigned int)(from - origin) * step;   /* j < W <= 65536; the product wraps mod 2^32 */
			const unsigned int i0 = (unsigned int)(from - k0), i1 = (unsigned int)(to - k0);
#pragma unroll 4
			for (unsigned int i = i0; i < i1; ++i) {
				const float w = wv[i];
				const unsigned int x = p >> 20;
				const float s = tab[x], c = tab[(x + 1024u) & (TN_TABLE - 1u)];
				I += (long long)(int)rintf(w * c);
				Q += (long long)(int)rintf(w * s);
				p += step;
			}
		}
		red[u][(seg * WR_LANES + lane) * 2u] = I;
		red[u][(seg * WR_LANES + lane) * 2u + 1u] = Q;
	}
#pragma unroll
	for (unsigned int d = WR_LANES / 2u; d; d >>= 1) {
		e_a += __shfl_down(e_a, d);
		e_b += __shfl_down(e_b, d);
	}
	if (lane == 0) {
		red_e[u][0] = e_a;
		red_e[u][1] = e_b;
	}
	__syncthreads();
	long long sum = 0;
#pragma unroll
	for (unsigned int j = 0; j < TN_WAVES; ++j)
		sum += red[j][tid];
	if (((tid >> 1) & (WR_LANES - 1u)) < ntones && sum)
		atomicAdd((unsigned long long *)&R->part[0][0][0] + tid, (unsigned long long)sum);
	if (tid < 2u) {
		long long e = 0;
#pragma unroll
		for (unsigned int j = 0; j < TN_WAVES; ++j)
			e += red_e[j][tid];
		if (e)
			atomicAdd((unsigned long long *)&R->part_e[tid], (unsigned long long)e);
	}
}

/* a workgroup of 64 lanes per row, a lane per tone: where a window ended in the push, A (joined with the carried sums
 * where that window began before the push) is latched and B becomes the carry; else B is added to the carry */
__global__ void __launch_bounds__(WR_LANES)
k_tones_latch(WrTonesRow *__restrict__ rows, unsigned long long nq, unsigned int nr, unsigned int W)
{
	WrTonesRow *R = rows + blockIdx.x;
	const unsigned int t = threadIdx.x;
	const unsigned int fill = R->fill;
	__syncthreads();                                              /* (lane 0 is about to change it) */
	const WrTonesCut cut = wrp_tones_cut(fill, nq, nr, W);
	const bool joined = cut.ends == 1u;                           /* (with fill = 0 the carried sums are 0) */
#pragma unroll
	for (unsigned int c = 0; c < 2u; ++c) {
		const long long a = R->part[0][t][c], b = R->part[1][t][c];
		if (cut.ends) {
			R->lat[t][c] = (joined ? R->acc[t][c] : 0) + a;
			R->acc[t][c] = b;
		} else {
			R->acc[t][c] += b;
		}
		R->part[0][t][c] = 0;
		R->part[1][t][c] = 0;
	}
	if (t == 0) {
		const long long a = R->part_e[0], b = R->part_e[1];
		if (cut.ends) {
			R->lat_e = (joined ? R->acc_e : 0) + a;
			R->acc_e = b;
		} else {
			R->acc_e += b;
		}
		R->part_e[0] = 0;
		R->part_e[1] = 0;
		R->windows += cut.ends;
		R->fill = cut.fill_after;
	}
}

hipError_t wrk_tones_push(hipStream_t st, const float *audio, size_t row_stride, size_t nrows, size_t nframes, WrTonesRow *rows,
                          const float *t12, const unsigned int *steps, unsigned int ntones, unsigned int window)
{
	if (!nrows || !nframes)
		return hipSuccess;
	if (!audio || !rows || !t12 || !steps || !ntones || ntones > WR_LANES || window < TN_WINDOW_MIN || window > TN_WINDOW_MAX ||
	    nrows > 65535u || (nrows > 1 && row_stride < nframes))
		return hipErrorInvalidValue;
	const WrTonesPlan g = wrp_tones_plan(nframes, window);
	if (g.chunks > 0x7fffffffu)
		return hipErrorInvalidValue;
	k_tones_part<<<dim3((unsigned int)g.chunks, (unsigned int)nrows), TN_THREADS, 0, st>>>(audio, row_stride, nframes, g.nq, g.nr,
	                                                                                       rows, t12, steps, ntones, window);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	k_tones_latch<<<(unsigned int)nrows, WR_LANES, 0, st>>>(rows, g.nq, g.nr, window);
	return hipGetLastError();
}
