/*
 * wr_dcs.hip -- a bank of up to 128 DCS (digital-coded squelch) code words over rows of audio (a tuner's audio[S][k2max]: one
 * row per channel slot; a plain block of rows): a bit slicer at 134.4 bit/s and a correlator over 23-bit words.  The rule is
 * include/webradio_amd.h's (wr_dcs_push_rows); with N the bank's ONE clock (frames so far) and `step` 134.4 Hz in units of
 * 2^-32 bit per frame:
 *
 *   frame n belongs to chip g(n) = floor(n * step / 2^29)                   eight chips per bit
 *   C[g] += (int64)rint(min(max(v', -64), 64) * 2^24)                       v' = 0 for an inf or a NaN
 *   evaluation e, once g(N) >= 8 e; for phase f = 0 .. 7:
 *     B_b = sum_{c < 8} C[8 e - 184 - f + 8 b + c],  b = 0 .. 22;   w_f = sum_b 2^b [2 B_b > max B + min B]
 *   agree[k] = max over f and the 23 rotations r of (23 - popcount(w_f ^ rot_r(word_k)), popcount(w_f ^ rot_r(word_k)))
 *
 * Every sum is one of INTEGERS: a stream has one result whatever the grid, the cut into pushes and the order of additions.
 *
 * State (WrDcsRow): a ring of DC_RING = 512 chip sums indexed by g mod 512, and agree / run / hits per code and polarity.
 * The open chip is simply the ring's entry g(N).  A launch takes frames whose chips, the next frame's included, lie within
 * DC_SPAN = 256 of its first; an evaluation reaches 191 chips back, so 191 + 256 < 512 ring entries are alive in a launch
 * and none is overwritten while it is still needed.  wrk_dcs_push cuts a longer push into several launches; the clock's
 * product beyond 2^64 is reduced there, on the host (ph0 = N0 * step mod 2^29, g0 = the first frame's chip), and the kernel
 * adds k * step < 2^56 for frame k of the launch.
 *
 * Mapping (k_dcs_push): A WORKGROUP OF 4 WAVES IS A ROW.
 *   1 the ring's live part comes into LDS (the chips that open in this launch as 0);
 *   2 chip sums: a wave reads 64 consecutive frames (coalesced), a segmented wave64 scan over lanes of equal chip adds them
 *     up, and the last lane of each run adds its sum to the LDS ring with one 64-bit integer atomic -- runs of different
 *     waves may share a chip; at 2 frames per chip that is 32 atomics to 32 addresses, at 46 (50 kHz) two or three;
 *   3 the chips the launch touched go back to the row's ring;
 *   4 per evaluation: thread (f, b) = (tid / 32, tid % 32), b < 23, sums its eight chips; the 32-lane half that is phase f
 *     reduces max and min by xor shuffles, a ballot is w_f, and thread (f, b) writes rot_b(w_f) -- the RECEIVED word is
 *     rotated once, not every code word -- to LDS: 184 candidates.  Then A LANE IS A CODE: thread t takes code t % 128
 *     and half t / 128 of the candidates (92 broadcast LDS reads, each an xor, a popcount, a max and a min), the halves
 *     meet in LDS, and lane k counts the evaluation into registers that go back to the row once, behind the last one.
 * LDS image of the ring: chip p sits at 8-byte word p + p / 8.  The eight-chip sums of a half start 8 chips = 64 bytes
 * apart, which on 64 banks of 4 bytes (ds_read_b64: bank = (a / 4) mod 64) would put lanes b and b + 4 on one bank; with a
 * pad word behind every eight chips they start 72 bytes = 18 banks apart and the 23 lanes of a half meet no bank twice.
 */
#include "wr_internal.h"
#include "wr_rows.h"

/* (DC_*, the start of a push and its cut into launches are wr_plan.h's) */
#define DC_SLOT(p) ((p) + ((p) >> 3))

__global__ void __launch_bounds__(DC_THREADS)
k_dcs_push(const float *__restrict__ audio, size_t row_stride, unsigned int nframes, WrDcsRow *__restrict__ rows,
           const unsigned int *__restrict__ words, unsigned int ncodes, unsigned int step, unsigned int ph0,
           unsigned long long g0, unsigned int max_errors)
{
	__shared__ long long ring[DC_SLOT(DC_RING)];
	__shared__ unsigned int cand[DC_CAND];
	__shared__ unsigned int other[WR_DCS_CODES];                  /* the upper half's (max << 8 | min) per code */
	const unsigned int tid = threadIdx.x, lane = tid & (WR_LANES - 1u);
	WrDcsRow *R = rows + blockIdx.x;
	const float *row = audio + (size_t)blockIdx.x * row_stride;
	/* chips g0 .. g0 + span are the launch's: g0 was open before it, the others open in it */
	const unsigned int span = (unsigned int)(((unsigned long long)ph0 + (unsigned long long)nframes * step) >> 29);
	const unsigned int r0 = (unsigned int)g0 & (DC_RING - 1u);

	/* 1: chips g0 - 191 .. g0 as the row has them, g0 + 1 .. g0 + span zero */
	for (unsigned int i = tid; i <= DC_BACK + span; i += DC_THREADS) {
		const unsigned int p = (r0 + i - DC_BACK) & (DC_RING - 1u);
		ring[DC_SLOT(p)] = i <= DC_BACK ? R->ring[p] : 0;
	}
	__syncthreads();

	/* 2: chip sums */
	for (unsigned int base = 0; base < nframes; base += DC_THREADS) {
		const unsigned int k = base + tid;
		const bool valid = k < nframes;
		long long q = 0;
		unsigned int c = 0xffffffffu;
		if (valid) {
			q = (long long)(int)rintf(row_fixed24(row[k]));
			c = (unsigned int)(((unsigned long long)ph0 + (unsigned long long)k * step) >> 29);
		}
#pragma unroll
		for (unsigned int d = 1; d < WR_LANES; d <<= 1) {         /* c does not fall from lane to lane: runs are contiguous */
			const long long oq = __shfl_up(q, d);
			const unsigned int oc = __shfl_up(c, d);
			if (lane >= d && oc == c)
				q += oq;
		}
		const unsigned int nc = __shfl_down(c, 1u);
		if (valid && (lane == WR_LANES - 1u || nc != c))
			atomicAdd((unsigned long long *)&ring[DC_SLOT((r0 + c) & (DC_RING - 1u))], (unsigned long long)q);
	}
	__syncthreads();

	/* 3: what changed goes back */
	for (unsigned int i = tid; i <= span; i += DC_THREADS) {
		const unsigned int p = (r0 + i) & (DC_RING - 1u);
		R->ring[p] = ring[DC_SLOT(p)];
	}

	/* 4: evaluations g0 / 8 + 1 .. (g0 + span) / 8 */
	const unsigned long long e0 = g0 >> 3;
	const unsigned int nev = (unsigned int)(((g0 + span) >> 3) - e0);
	if (!nev)
		return;
	const unsigned int code = tid & (WR_DCS_CODES - 1u), half = tid / WR_DCS_CODES;
	const bool mine = half == 0 && code < ncodes;
	const unsigned int word = code < ncodes ? words[code] : 0u;
	unsigned int agree[2] = {0, 0}, run[2] = {0, 0};
	unsigned long long hits[2] = {0, 0};
	if (mine) {
#pragma unroll
		for (unsigned int pol = 0; pol < 2u; ++pol) {
			run[pol] = R->run[code][pol];
			hits[pol] = R->hits[code][pol];
		}
	}
	const unsigned int f = tid >> 5, b = tid & 31u;
	for (unsigned int ev = 0; ev < nev; ++ev) {
		/* chip 8 e, relative to the ring */
		const unsigned int at = (unsigned int)((e0 + 1u + ev) << 3);
		long long B = 0;
		if (b < 23u) {
			const unsigned int p0 = at - 184u - f + 8u * b;
#pragma unroll
			for (unsigned int c = 0; c < 8u; ++c) {
				const unsigned int p = (p0 + c) & (DC_RING - 1u);
				B += ring[DC_SLOT(p)];
			}
		}
		long long hi = b < 23u ? B : (long long)0x8000000000000000ull, lo = b < 23u ? B : 0x7fffffffffffffffll;
#pragma unroll
		for (unsigned int d = 16u; d; d >>= 1) {
			const long long oh = __shfl_xor(hi, d, 32), ol = __shfl_xor(lo, d, 32);
			hi = oh > hi ? oh : hi;
			lo = ol < lo ? ol : lo;
		}
		const unsigned long long set = __ballot(b < 23u && 2 * B > hi + lo);
		const unsigned int w = (unsigned int)(set >> (32u * (f & 1u))) & 0x7fffffu;
		if (b < 23u)
			cand[f * 23u + b] = ((w << b) | (w >> (23u - b))) & 0x7fffffu;
		__syncthreads();
		unsigned int most = 0, least = 23u;
#pragma unroll 4
		for (unsigned int i = 0; i < DC_CAND / 2u; ++i) {
			const unsigned int x = __popc(cand[half * (DC_CAND / 2u) + i] ^ word);
			most = x > most ? x : most;
			least = x < least ? x : least;
		}
		if (half)
			other[code] = (most << 8) | least;
		__syncthreads();
		if (mine) {
			const unsigned int o = other[code];
			most = (o >> 8) > most ? (o >> 8) : most;
			least = (o & 255u) < least ? (o & 255u) : least;
			agree[0] = 23u - least;
			agree[1] = most;
#pragma unroll
			for (unsigned int pol = 0; pol < 2u; ++pol) {
				const bool match = agree[pol] + max_errors >= 23u;
				hits[pol] += match ? 1u : 0u;
				run[pol] = match ? run[pol] + 1u : 0u;
			}
		}
	}
	if (mine) {
#pragma unroll
		for (unsigned int pol = 0; pol < 2u; ++pol) {
			R->agree[code][pol] = (unsigned char)agree[pol];
			R->run[code][pol] = run[pol];
			R->hits[code][pol] = hits[pol];
		}
	}
	if (tid == 0)
		R->evals += nev;
}

hipError_t wrk_dcs_push(hipStream_t st, const float *audio, size_t row_stride, size_t nrows, size_t nframes, WrDcsRow *rows,
                        const unsigned int *words, unsigned int ncodes, unsigned int step, unsigned long long first_frame,
                        unsigned int max_errors)
{
	if (!nrows || !nframes)
		return hipSuccess;
	if (!audio || !rows || !words || !ncodes || ncodes > WR_DCS_CODES || !wrp_dcs_step_ok(step) || max_errors > 3u ||
	    nrows > 65535u || nframes > ((size_t)1 << 28) || (nrows > 1 && row_stride < nframes))
		return hipErrorInvalidValue;
	WrDcsAt at = wrp_dcs_start(first_frame, step);
	for (size_t done = 0, n; done < nframes; done += n, at = wrp_dcs_after(at, step, n)) {
		n = wrp_dcs_take(at, step, nframes - done);
		k_dcs_push<<<(unsigned int)nrows, DC_THREADS, 0, st>>>(audio + done, row_stride, (unsigned int)n, rows, words, ncodes, step,
		                                                       at.ph0, at.g0, max_errors);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess)
			return e;
	}
	return hipSuccess;
}
