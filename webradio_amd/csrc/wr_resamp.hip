/*
 * wr_resamp.hip -- a rational polyphase resampler over rows of audio (a tuner's audio[S][k2max]: one row per channel slot; a
 * plain block of rows): every row by the same ratio L / M with P taps per phase.  The rule is include/webradio_amd.h's
 * (wr_resamp_push_rows); output frame m of a row's stream x (cleaned: x'), with t = m * M, n0 = t / L, ph = t mod L:
 *
 *   acc = +0.0f;  for k = 0 ... P-1:  acc = acc + c[ph][k] * x'[n0 - k];  y[m] = acc
 *
 * -- one float32 product and one float32 sum per tap, in this order, nothing fused (the file is compiled with
 * -ffp-contract=off), so an output has one value whatever the grid and the cut into pushes.
 *
 * What a push of n frames at clock N0 (only r = N0 mod M is kept) holds: with j0 = ceil(r L / M), output i of the push is
 * frame m = q L + j0 + i of the stream (N0 = q M + r), so t = q L M + (j0 + i) M and, counted from the push's first frame,
 * n0 - N0 = (j0 + i) M / L - r >= 0 and ph = (j0 + i) M mod L.  The push yields ceil((r + n) L / M) - j0 outputs, each of
 * which has n0 - N0 < n.
 *
 * Mapping (k_resamp_rows): the grid is (chunks + 1) x rows.  A workgroup of 256 threads is 256 consecutive outputs of one
 * row: ONE 64-bit division per workgroup gives the chunk's first (n0 - N0, ph); a thread adds tid * M in 32 bits.  The input
 * span of the chunk -- (rem0 + 255 M) / L + P frames, at most 2 104 -- is staged into LDS, cleaned on the way in, from the
 * row's history where it reaches in front of the push.  A thread reads its phase's P taps as float4 through the cache
 * (the table is at most 64 KiB) and walks k in order.  The LAST workgroup of a row (blockIdx.x == chunks) writes the row's
 * new history -- the last P - 1 frames of old history ++ push -- into the OTHER history set, so no workgroup of the push
 * reads what another writes; the host takes the sets in turn.
 */
#include "wr_internal.h"
#include "wr_rows.h"

/* (RS_*, the limits RS_SPAN rests on, the figures of a push and of a chunk -- wrp_resamp_chunk -- are wr_plan.h's) */

__global__ void __launch_bounds__(RS_THREADS)
k_resamp_rows(const float *__restrict__ in, size_t row_stride, unsigned int nframes, const float *__restrict__ taps,
              unsigned int L, unsigned int M, unsigned int P, const float *__restrict__ hist_old, float *__restrict__ hist_new,
              unsigned int nmod, unsigned int j0, unsigned long long n_out, unsigned int chunks, float *__restrict__ out,
              size_t out_stride)
{
	__shared__ float xs[RS_SPAN];
	const unsigned int tid = threadIdx.x, H = P - 1u;
	const float *row = in + (size_t)blockIdx.y * row_stride;
	const float *ho = hist_old + (size_t)blockIdx.y * H;
	if (blockIdx.x == chunks) {                                   /* the row's new history: frames [nframes - H, nframes) */
		if (tid < H) {
			const long long n = (long long)nframes - (long long)H + (long long)tid;
			hist_new[(size_t)blockIdx.y * H + tid] = n < 0 ? ho[(long long)H + n] : row_clean(row[n]);
		}
		return;
	}
	const WrResampChunk ch = wrp_resamp_chunk(L, M, P, nmod, j0, n_out, blockIdx.x);
	const unsigned long long i0 = ch.i0;
	const unsigned int rem0 = ch.rem0, cnt = ch.cnt;
	const long long lo = ch.lo;                                   /* xs[i] is frame lo + i of the push; lo >= -H */
	for (unsigned int i = tid; i < ch.span; i += RS_THREADS) {
		const long long n = lo + (long long)i;
		xs[i] = n < 0 ? ho[(long long)H + n] : n < (long long)nframes ? row_clean(row[n]) : 0.0f;
	}
	__syncthreads();
	if (tid >= cnt)
		return;
	const unsigned int v = rem0 + tid * M;                        /* < L + 255 * 8 L: 32 bits hold it */
	const unsigned int q = v / L, ph = v - q * L;
	const float4 *c = (const float4 *)(taps + (size_t)ph * P);
	const float *x = xs + q + H;                                  /* x[-k] = x'[n0 - k] */
	float acc = 0.0f;
	for (unsigned int k = 0; k < P; k += 4u) {
		const float4 t = c[k >> 2];
		acc = acc + t.x * x[-(int)k];
		acc = acc + t.y * x[-(int)k - 1];
		acc = acc + t.z * x[-(int)k - 2];
		acc = acc + t.w * x[-(int)k - 3];
	}
	out[(size_t)blockIdx.y * out_stride + i0 + tid] = acc;
}

unsigned long long wrk_resamp_out_frames(unsigned int L, unsigned int M, unsigned int nmod, unsigned long long nframes)
{
	return wrp_resamp_out_frames(L, M, nmod, nframes);
}

hipError_t wrk_resamp_push(hipStream_t st, const float *in, size_t row_stride, size_t nrows, size_t nframes, const WrResampPush &p,
                           float *out, size_t out_stride)
{
	if (!nrows || !nframes)
		return hipSuccess;
	if (!in || !p.taps || !p.hist_old || !p.hist_new || p.hist_old == p.hist_new || wrd_resamp_limits(p.L, p.M, p.P) ||
	    p.nmod >= p.M || nrows > 65535u || nframes > ((size_t)1 << 28) || (nrows > 1 && row_stride < nframes))
		return hipErrorInvalidValue;
	const WrResampPlan g = wrp_resamp_plan(p.L, p.M, p.nmod, nframes);
	if (g.n_out && (!out || (nrows > 1 && out_stride < g.n_out)))
		return hipErrorInvalidValue;
	k_resamp_rows<<<dim3(g.grid_x, (unsigned int)nrows), RS_THREADS, 0, st>>>(in, row_stride, (unsigned int)nframes, p.taps, p.L, p.M,
	                                                                          p.P, p.hist_old, p.hist_new, p.nmod, g.j0, g.n_out,
	                                                                          g.chunks, out, out_stride);
	return hipGetLastError();
}
