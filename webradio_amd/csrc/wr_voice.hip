/*
 * wr_voice.hip -- the voice bank: one long FIR filter per row of audio, chosen per row from a table of up to 16 filters of ONE
 * length T, and a mute.  The rule is include/webradio_amd.h's (wr_voice_push_rows); output frame n of a row's stream x
 * (cleaned: x') on filter f:
 *
 *   acc = +0.0f;  for k = 0 ... T-1:  acc = acc + c[f][k] * x'[n - k];  y[n] = mute ? +0.0f : acc
 *
 * -- one float32 product and one float32 sum per tap, in this order, nothing fused (the file is compiled with
 * -ffp-contract=off), so an output has one value whatever the grid and the cut into pushes.
 *
 * Mapping (k_voice_rows): the grid is (chunks + 1) x rows (wrp_voice_plan).  A workgroup -- one wave -- is VOICE_CHUNK
 * consecutive outputs of ONE row, so the row's control word, its filter and with it every tap are uniform: the taps come
 * through the scalar cache, sixteen to a load, asked for a turn ahead.  The chunk's input span, VOICE_CHUNK + T - 1 frames,
 * is staged into LDS, cleaned on the way in, from the row's history where it reaches in front of the push.  A thread owns
 * VOICE_PER = 4 consecutive outputs o ... o + 3: four accumulators and a window of the inputs x'[o - k - 3 ... o - k + 3] in
 * registers.  Four taps k ... k + 3 cost 16 products and 16 sums on that window and ONE 128-bit LDS read, the four inputs in
 * front of it, which is issued a step ahead; the window then slides by renaming (sixteen registers, a turn every four
 * steps), without a move.  Within an output k is walked in order.  Lanes lie four dwords apart: every 128-bit read is
 * 16-byte aligned and conflict-free.
 * Why four and not eight outputs a thread (measured, profiles/voice.txt): a wave's time is its 2 T VOICE_PER instructions,
 * one behind the other, whatever the grid -- a push of 256 rows of 2 000 frames is a thousand waves of eight outputs, ONE per
 * SIMD, and two thousand of four run faster (36.5 against 42.1 us at 1024 taps), as they do at 512 rows (59.1 / 66.6) and
 * 1024 (97.7 / 99.0); eight outputs win only from 2048 rows on, by 2.5 %.  Two outputs a thread would put odd lanes off
 * 16-byte alignment.
 * The outputs go out through LDS, so that lanes store neighbouring floats.
 * The LAST workgroup of a row (blockIdx.x == chunks) writes the row's new history -- the last T - 1 frames of old
 * history ++ push -- into the OTHER history set, so no workgroup of the push reads what another writes; the host takes the
 * sets in turn.  A muted row's chunks store zeros; its history is written like any other's.
 */
#include "wr_internal.h"
#include "wr_rows.h"

static_assert(VOICE_CHUNK == VOICE_THREADS * VOICE_PER, "a chunk is every thread's outputs");
static_assert(VOICE_PER % 4u == 0 && VOICE_PER <= 8u && VOICE_THREADS == WR_LANES,
              "k_voice_rows: lanes read 16-byte aligned, a window of sixteen registers holds at most eight outputs' inputs, a workgroup is one wave");
constexpr int PER = (int)VOICE_PER;

/* dst[i] = src[i] -- CLEAN: cleaned -- for i < n, lane `tid` every VOICE_THREADS-th of them; a lane has eight loads in flight
 * (a workgroup is one wave: nobody else hides a load's latency) */
template <bool CLEAN> __device__ __forceinline__ void vo_copy(float *dst, const float *__restrict__ src, unsigned int n, unsigned int tid)
{
	for (unsigned int i = tid; i < n; i += 8u * VOICE_THREADS) {
		float v[8];
#pragma unroll
		for (unsigned int j = 0; j < 8u; ++j) {
			const unsigned int at = i + j * VOICE_THREADS;
			v[j] = src[at < n ? at : n - 1u];                     /* (a load past the end: the last one again, and not stored) */
		}
#pragma unroll
		for (unsigned int j = 0; j < 8u; ++j)
			if (i + j * VOICE_THREADS < n)
				dst[i + j * VOICE_THREADS] = CLEAN ? row_clean(v[j]) : v[j];
	}
}

/* Step S (mod 4) of a thread: the taps t = c[k ... k + 3] on the window W[i] = x'[o - k - 3 + i], which lives in p[(i - 4 S) & 15];
 * `ahead` points at x'[o - k - 7], the next step's W[0 ... 3], which go into the four registers this step does not read. */
template <int S> __device__ __forceinline__ void vo_step(float (&acc)[PER], float (&p)[16], const float4 t, const float *ahead)
{
	const float4 nx = *(const float4 *)ahead;
	p[(0 - 4 * (S + 1)) & 15] = nx.x;
	p[(1 - 4 * (S + 1)) & 15] = nx.y;
	p[(2 - 4 * (S + 1)) & 15] = nx.z;
	p[(3 - 4 * (S + 1)) & 15] = nx.w;
#pragma unroll
	for (int j = 0; j < PER; ++j)
		acc[j] = acc[j] + t.x * p[(3 + j - 4 * S) & 15];
#pragma unroll
	for (int j = 0; j < PER; ++j)
		acc[j] = acc[j] + t.y * p[(2 + j - 4 * S) & 15];
#pragma unroll
	for (int j = 0; j < PER; ++j)
		acc[j] = acc[j] + t.z * p[(1 + j - 4 * S) & 15];
#pragma unroll
	for (int j = 0; j < PER; ++j)
		acc[j] = acc[j] + t.w * p[(0 + j - 4 * S) & 15];
}

__global__ void __launch_bounds__(VOICE_THREADS)
k_voice_rows(const float *__restrict__ in, size_t row_stride, unsigned int nframes, const float *__restrict__ taps, unsigned int T,
             const unsigned int *__restrict__ ctl, const float *__restrict__ hist_old, float *__restrict__ hist_new,
             unsigned int chunks, float *__restrict__ out, size_t out_stride)
{
	constexpr unsigned int CHUNK = VOICE_CHUNK;
	__shared__ __attribute__((aligned(16))) float lds[VOICE_LDS_FLOATS];
	float *xs = lds + 4;                                          /* xs[i] is frame lo + i of the push; xs[-4 ... -1]: read, never used */
	const unsigned int tid = threadIdx.x, H = T - 1u;
	const float *row = in + (size_t)blockIdx.y * row_stride;
	const float *ho = hist_old + (size_t)blockIdx.y * H;
	if (blockIdx.x == chunks) {                                   /* the row's new history: frames [nframes - H, nframes) */
		float *hn = hist_new + (size_t)blockIdx.y * H;
		const unsigned int keep = nframes < H ? H - nframes : 0u;   /* entries that stay old history (clean already) */
		vo_copy<false>(hn, ho + nframes, keep, tid);
		vo_copy<true>(hn + keep, row + (nframes + keep - H), H - keep, tid);
		return;
	}
	const unsigned int word = ctl[blockIdx.y];
	const unsigned int c0 = blockIdx.x * CHUNK;                   /* < 2^28 */
	const unsigned int left = nframes - c0;
	const unsigned int cnt = left < CHUNK ? left : CHUNK;
	float acc[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j)
		acc[j] = 0.0f;
	if (!(word & 0x100u)) {                                       /* (uniform: a muted row computes nothing) */
		/* the span: frames [c0 - H, c0 + cnt) of the push, the first `old` of them from the history (clean already) */
		const unsigned int span = cnt + H, all = CHUNK + T; /* behind the span: zeros, for the outputs nobody stores */
		const unsigned int old = c0 < H ? H - c0 : 0u;
		if (tid < 4u)
			lds[tid] = 0.0f;
		vo_copy<false>(xs, ho + c0, old, tid);
		vo_copy<true>(xs + old, row + (c0 + old - H), span - old, tid);
		for (unsigned int i = span + tid; i < all; i += VOICE_THREADS)
			xs[i] = 0.0f;
		__syncthreads();
		const float *c = taps + (size_t)(word & 0xffu) * T;
		const float *xp = xs + tid * PER + T - 4u;          /* x'[o - 3] of the thread's first output o; 16-byte aligned */
		float p[16];
#pragma unroll
		for (int i = 0; i < 16; ++i)
			p[i] = 0.0f;
#pragma unroll
		for (int i = 0; i < (PER + 6) / 4; ++i) {                 /* the first window, W[0 ... PER + 2]: the last float read is xs[CHUNK + T - 1] */
			const float4 w = *(const float4 *)(xp + 4 * i);
			p[4 * i] = w.x;
			p[4 * i + 1] = w.y;
			p[4 * i + 2] = w.z;
			p[4 * i + 3] = w.w;
		}
		/* sixteen taps a turn, the next turn's sixteen asked for before this turn's arithmetic: a wave has its SIMD to itself
		 * more often than not, and nobody else would hide the scalar cache's latency */
		unsigned int k = 0;
		float4 ta = make_float4(0.0f, 0.0f, 0.0f, 0.0f), tb = ta, tc = ta, td = ta;
		if (T >= 16u) {
			ta = *(const float4 *)c;
			tb = *(const float4 *)(c + 4);
			tc = *(const float4 *)(c + 8);
			td = *(const float4 *)(c + 12);
		}
		for (; k + 16u <= T; k += 16u) {
			float4 na = ta, nb = tb, nc = tc, nd = td;
			if (k + 32u <= T) {
				na = *(const float4 *)(c + k + 16u);
				nb = *(const float4 *)(c + k + 20u);
				nc = *(const float4 *)(c + k + 24u);
				nd = *(const float4 *)(c + k + 28u);
			}
			vo_step<0>(acc, p, ta, xp - k - 4u);
			vo_step<1>(acc, p, tb, xp - k - 8u);
			vo_step<2>(acc, p, tc, xp - k - 12u);
			vo_step<3>(acc, p, td, xp - k - 16u);
			ta = na;
			tb = nb;
			tc = nc;
			td = nd;
		}
		if (k + 4u <= T)
			vo_step<0>(acc, p, *(const float4 *)(c + k), xp - k - 4u);
		if (k + 8u <= T)
			vo_step<1>(acc, p, *(const float4 *)(c + k + 4u), xp - k - 8u);
		if (k + 12u <= T)
			vo_step<2>(acc, p, *(const float4 *)(c + k + 8u), xp - k - 12u);
		__syncthreads();                                          /* every window has been read: the stage becomes the outputs */
	}
	float4 *ys = (float4 *)(xs + tid * PER);
#pragma unroll
	for (int j = 0; j < PER / 4; ++j)
		ys[j] = make_float4(acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]);
	__syncthreads();
	float *y = out + (size_t)blockIdx.y * out_stride + c0;
	for (unsigned int i = tid; i < cnt; i += VOICE_THREADS)
		y[i] = xs[i];
}

hipError_t wrk_voice_push(hipStream_t st, const float *in, size_t row_stride, size_t nrows, size_t nframes, const WrVoicePush &p,
                          float *out, size_t out_stride)
{
	if (!nrows || !nframes)
		return hipSuccess;
	if (!in || !out || !p.taps || !p.ctl || !p.hist_old || !p.hist_new || p.hist_old == p.hist_new || !wrp_voice_len_ok(p.T) ||
	    nrows > 65535u || nframes > ((size_t)1 << 28) || (nrows > 1 && (row_stride < nframes || out_stride < nframes)))
		return hipErrorInvalidValue;
	const WrVoicePlan g = wrp_voice_plan(nframes);
	k_voice_rows<<<dim3(g.grid_x, (unsigned int)nrows), g.threads, 0, st>>>(in, row_stride, (unsigned int)nframes, p.taps, p.T, p.ctl,
	                                                                        p.hist_old, p.hist_new, g.chunks, out, out_stride);
	return hipGetLastError();
}
