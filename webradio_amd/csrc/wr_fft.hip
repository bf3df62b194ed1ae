/*
 * wr_fft.hip -- SpectrumSink on gfx950: Hamming window, forward complex FFT,
 * power -> dB with fftshift (io/spectrumsink.cxx:88-123 process, :125-142
 * getSpectrum).  Hand-written radix-2 Stockham transforms that live in LDS; no
 * rocFFT/hipFFT.
 *
 *   n <= 8192 : one workgroup per frame, the whole frame ping-pongs between two
 *               LDS buffers (2 x 64 KiB at n = 8192).
 *   n  > 8192 : four-step.  n = n1*n2, sample index n1*N2 + n2, bin k1 + N1*k2.
 *               pass 1: a workgroup takes CT adjacent columns n2, transforms them
 *                       over n1 in LDS, applies the window on load and the
 *                       inter-pass twiddle W_n^(n2*k1) on store -> work[k1][n2]
 *               pass 2: a workgroup takes RT adjacent rows k1, transforms them
 *                       over n2, writes bins (or dB, shifted) at k1 + N1*k2.
 *               For the 65536-point waterfall of BASELINE config 3 that is
 *               256 x 256 with one 512 KiB intermediate per frame, which stays in
 *               L2 / Infinity Cache between the passes.
 *
 * Real input (one channel: a receiver's audio; the reference's FIXMEs at io/spectrumsink.cxx:62-64): the n samples are
 * packed as m = n/2 complex points z[i] = (w[2i]*x[2i], w[2i+1]*x[2i+1]), the m-point transform Z runs on the machinery
 * above, and the untangle step X[k] = E - i*W_n^k*O, E/O = (Z[k] +/- conj(Z[m-k]))/2, X[n-k] = conj(X[k]) gives the n bins.
 *   n <= 16384 : one workgroup per frame, untangled out of the LDS result buffer.
 *   n  > 16384 : four-step on m, then k_fft_untangle.
 *
 * Mean and peak hold over the frames of a block (wr_spectrum_batch_avg): the transforms above write bins, k_spec_reduce
 * walks them frame by frame in one order of operations; k_rows_waterfall reduces dB rows to pixel rows.
 *
 * The window multiply is the reference's float multiply on the raw sample
 * (spectrumsink.cxx:109-112); the dB expression is the reference's float
 * expression (spectrumsink.cxx:127,137-138).
 */
#include "wr_internal.h"

#include <cstdlib>
#include <cstring>
#include <vector>

/* (FFT_THREADS, the LDS budget and every other figure of the launches: wr_plan.h) */

__device__ __forceinline__ float2 cmul(float2 a, float2 w)
{
	return make_float2(__builtin_fmaf(a.x, w.x, -a.y * w.y), __builtin_fmaf(a.x, w.y, a.y * w.x));
}

/* `ncols` independent length-`len` transforms, element (i, col) at buf[i*ncols + col].
 * Radix-2 Stockham autosort: natural order in, natural order out.  tw is the table
 * exp(-2*pi*i*k/(len*scale)), k < len*scale/2 (a table for a longer transform is the
 * same table sampled `scale` times finer).  Returns the buffer holding the result. */
__device__ float2 *lds_fft(float2 *a, float2 *b, unsigned int len, unsigned int ncols,
                           const float2 *__restrict__ tw, unsigned int scale, unsigned int tid)
{
	const unsigned int half = len >> 1;
	const unsigned int total = half * ncols;
	float2 *in = a, *out = b;
	for (unsigned int ns = 1; ns < len; ns <<= 1) {
		const unsigned int twstep = (half / ns) * scale;   /* len*scale / (2*ns) */
		for (unsigned int t = tid; t < total; t += FFT_THREADS) {
			const unsigned int j = t / ncols;
			const unsigned int col = t - j * ncols;
			const unsigned int k = j & (ns - 1);
			const float2 w = tw[k * twstep];
			const float2 v0 = in[j * ncols + col];
			const float2 v1 = cmul(in[(j + half) * ncols + col], w);
			const unsigned int j0 = ((j - k) << 1) + k;
			out[j0 * ncols + col] = make_float2(v0.x + v1.x, v0.y + v1.y);
			out[(j0 + ns) * ncols + col] = make_float2(v0.x - v1.x, v0.y - v1.y);
		}
		__syncthreads();
		float2 *tmp = in;
		in = out;
		out = tmp;
	}
	return in;
}

__device__ __forceinline__ float to_db(float2 v, float scaledb)
{
	/* spectrumsink.cxx:137-138: 10*log10f(re*re + im*im) - 20*log10f(N) */
	return 10.0f * log10f(v.x * v.x + v.y * v.y) - scaledb;
}

/* where frame `frame` of a launch starts, in frames from the input pointer: frame f of group g at g * gstride + f * hop,
 * `fpg` frames per group (one group: fpg = the launch's frames, and this is frame * hop) */
__device__ __forceinline__ size_t frame_start(size_t frame, size_t hop, unsigned int fpg, size_t gstride)
{
	const size_t g = frame / fpg;
	return g * gstride + (frame - g * fpg) * hop;
}

/* whole frame in LDS; grid.x = frame (group-major: wr_spectrum_batch_avg's groups share one launch) */
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_single(const float2 *__restrict__ iq, size_t hop, unsigned int fpg, size_t gstride, unsigned int n,
             const float *__restrict__ window, const float2 *__restrict__ tw,
             float2 *__restrict__ bins, float *__restrict__ db, float scaledb)
{
	extern __shared__ float2 lds[];
	float2 *a = lds, *b = lds + n;
	const size_t frame = blockIdx.x;
	const float2 *x = iq + frame_start(frame, hop, fpg, gstride);
	for (unsigned int i = threadIdx.x; i < n; i += FFT_THREADS) {
		const float2 v = x[i];
		const float w = window[i];
		a[i] = make_float2(v.x * w, v.y * w);
	}
	__syncthreads();
	const float2 *r = lds_fft(a, b, n, 1, tw, 1, threadIdx.x);
	for (unsigned int k = threadIdx.x; k < n; k += FFT_THREADS) {
		const float2 v = r[k];
		if (bins)
			bins[frame * n + k] = v;
		if (db)
			db[frame * n + ((k + (n >> 1)) & (n - 1))] = to_db(v, scaledb);
	}
}

/* CT adjacent columns of a [rows][S] array of IQ frames (a tuner's channel IQ: one lane per channel slot), rows
 * `first` ... `first + n - 1`: one n-point frame per column, all of them in LDS side by side as lds_fft wants them,
 * a[i*CT + c].  grid.x = cols / ct: the first `cols` columns (the launcher's ct divides 64, cols is whole lane groups).  Load: adjacent lanes read
 * adjacent slots of one row, ct * 8 bytes contiguous.  Store: the bin index runs fastest, so a wave writes runs of ONE
 * dB row (whole 256-byte runs from n = 64 on) and reads LDS with a stride of ct points: the global stores are what is
 * kept coalesced, the LDS reads take the bank conflicts (none at ct = 1). */
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_cols(const float2 *__restrict__ iq, unsigned int S, unsigned int cols, size_t first, unsigned int n, unsigned int ct,
           const float *__restrict__ window, const float2 *__restrict__ tw, float *__restrict__ db, float scaledb)
{
	extern __shared__ float2 lds[];
	const unsigned int total = n * ct;
	float2 *a = lds, *b = lds + total;
	const unsigned int slot0 = blockIdx.x * ct;
	const unsigned int lgct = 31u - (unsigned int)__builtin_clz(ct), lgn = 31u - (unsigned int)__builtin_clz(n);
	const float2 *x = iq + first * S;
	for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const unsigned int i = e >> lgct, slot = slot0 + (e & (ct - 1u));
		const float2 v = slot < cols ? x[(size_t)i * S + slot] : make_float2(0.0f, 0.0f);
		const float w = window[i];
		a[e] = make_float2(v.x * w, v.y * w);               /* spectrumsink.cxx:109-112 */
	}
	__syncthreads();
	const float2 *r = lds_fft(a, b, n, ct, tw, 1, threadIdx.x);
	for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const unsigned int c = e >> lgn, k = e & (n - 1u), slot = slot0 + c;
		if (slot < cols)
			db[(size_t)slot * n + ((k + (n >> 1)) & (n - 1u))] = to_db(r[k * ct + c], scaledb);
	}
}

/* a packed point of a real frame: samples 2i and 2i+1, windowed.  A frame starts at any float offset (any hop, pushes of
 * any length), so the pair is one 8-byte load only where the frame happens to be 8-byte aligned. */
__device__ __forceinline__ float2 real_pair(const float *__restrict__ x, bool aligned, const float *__restrict__ window,
                                            unsigned int i)
{
	float2 v;
	if (aligned)
		v = *(const float2 *)(x + 2u * i);
	else
		v = make_float2(x[2u * i], x[2u * i + 1u]);
	const float2 w = *(const float2 *)(window + 2u * i);
	return make_float2(v.x * w.x, v.y * w.y);
}

/* bin k of a real frame of 2m samples from Z[k], Z[m-k] of its packed transform and w = W_2m^k, 0 < k < m */
__device__ __forceinline__ float2 untangle(float2 zk, float2 zr, float2 w)
{
	const float2 e = make_float2(0.5f * (zk.x + zr.x), 0.5f * (zk.y - zr.y));   /* (Z[k] + conj(Z[m-k])) / 2 */
	const float2 o = make_float2(0.5f * (zk.x - zr.x), 0.5f * (zk.y + zr.y));   /* (Z[k] - conj(Z[m-k])) / 2 */
	const float2 t = cmul(o, w);
	return make_float2(e.x + t.y, e.y - t.x);                                   /* E - i*W*O */
}

/* bins k and n-k of frame `fbase / n` (Hermitian completion), or their dB values at the shifted positions */
__device__ __forceinline__ void put_real_bins(float2 *__restrict__ bins, float *__restrict__ db, size_t fbase,
                                              unsigned int n, unsigned int k, float2 zk, float2 zr, float2 w, float scaledb)
{
	const unsigned int m = n >> 1;
	if (k == 0) {
		/* X[0] and X[m] are Re Z0 +/- Im Z0 */
		const float2 x0 = make_float2(zk.x + zk.y, 0.0f), xm = make_float2(zk.x - zk.y, 0.0f);
		if (bins) {
			bins[fbase] = x0;
			bins[fbase + m] = xm;
		}
		if (db) {
			db[fbase + m] = to_db(x0, scaledb);
			db[fbase] = to_db(xm, scaledb);
		}
		return;
	}
	const float2 v = untangle(zk, zr, w);
	if (bins) {
		bins[fbase + k] = v;
		bins[fbase + n - k] = make_float2(v.x, -v.y);
	}
	if (db) {
		const float d = to_db(v, scaledb);
		db[fbase + m + k] = d;
		db[fbase + m - k] = d;
	}
}

/* a real frame of n <= 16384 samples whole in LDS (m = n/2 packed points); grid.x = frame (group-major, frame_start),
 * `hop` and `gstride` in floats */
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_real_single(const float *__restrict__ in, size_t hop, unsigned int fpg, size_t gstride, unsigned int n,
                  const float *__restrict__ window, const float2 *__restrict__ tw,
                  float2 *__restrict__ bins, float *__restrict__ db, float scaledb)
{
	extern __shared__ float2 lds[];
	const unsigned int m = n >> 1;
	float2 *a = lds, *b = lds + m;
	const size_t frame = blockIdx.x;
	const float *x = in + frame_start(frame, hop, fpg, gstride);
	const bool aligned = ((size_t)x & 7u) == 0;
	for (unsigned int i = threadIdx.x; i < m; i += FFT_THREADS)
		a[i] = real_pair(x, aligned, window, i);
	__syncthreads();
	const float2 *r = lds_fft(a, b, m, 1, tw, 2, threadIdx.x);     /* (tw is the n-point table: every other entry) */
	for (unsigned int k = threadIdx.x; k < m; k += FFT_THREADS)
		put_real_bins(bins, db, frame * n, n, k, r[k], r[(m - k) & (m - 1)], tw[k], scaledb);
}

/* the untangle step behind pass 2 of a real frame's packed transform; grid = (m/256, frames) */
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_untangle(const float2 *__restrict__ z, unsigned int n, const float2 *__restrict__ tw,
               float2 *__restrict__ bins, float *__restrict__ db, float scaledb)
{
	const unsigned int m = n >> 1;
	const unsigned int k = blockIdx.x * FFT_THREADS + threadIdx.x;
	const size_t frame = blockIdx.y;
	const float2 *zf = z + frame * m;
	if (k < m)
		put_real_bins(bins, db, frame * n, n, k, zf[k], zf[(m - k) & (m - 1)], tw[k], scaledb);
}

/* four-step pass 1; grid = (n2/ct, frames).  REAL: `iq` are floats, `hop` counts floats, the transform is the packed one
 * of n1*n2 points and tw_n the table of TWICE that size */
template <bool REAL>
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_pass1(const float2 *__restrict__ iq, size_t hop, unsigned int n1, unsigned int n2,
            unsigned int ct, const float *__restrict__ window, const float2 *__restrict__ tw_sub,
            unsigned int tw_sub_len, const float2 *__restrict__ tw_n, float2 *__restrict__ work)
{
	extern __shared__ float2 lds[];
	const unsigned int n = n1 * n2;
	float2 *a = lds, *b = lds + (size_t)n1 * ct;
	const size_t frame = blockIdx.y;
	const unsigned int col0 = blockIdx.x * ct;
	const unsigned int total = n1 * ct;
	if (REAL) {
		const float *x = (const float *)iq + frame * hop;
		const bool aligned = ((size_t)x & 7u) == 0;
		for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
			const unsigned int r = e / ct, c = e - r * ct;
			a[e] = real_pair(x, aligned, window, r * n2 + col0 + c);
		}
	} else {
		const float2 *x = iq + frame * hop;
		for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
			const unsigned int r = e / ct, c = e - r * ct;
			const unsigned int idx = r * n2 + col0 + c;
			const float2 v = x[idx];
			const float w = window[idx];
			a[e] = make_float2(v.x * w, v.y * w);
		}
	}
	__syncthreads();
	const float2 *res = lds_fft(a, b, n1, ct, tw_sub, tw_sub_len / n1, threadIdx.x);
	float2 *wout = work + frame * n;
	for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const unsigned int k1 = e / ct, c = e - k1 * ct;
		const unsigned int col = col0 + c;
		unsigned int m = col * k1;                      /* < n */
		float2 w;
		if (m < (n >> 1)) {
			w = tw_n[REAL ? 2u * m : m];
		} else {
			const float2 t = tw_n[REAL ? 2u * (m - (n >> 1)) : m - (n >> 1)];
			w = make_float2(-t.x, -t.y);
		}
		wout[(size_t)k1 * n2 + col] = cmul(res[e], w);
	}
}

/* four-step pass 2; grid = (n1/rt, frames) */
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_pass2(const float2 *__restrict__ work, unsigned int n1, unsigned int n2, unsigned int rt,
            const float2 *__restrict__ tw_sub, unsigned int tw_sub_len,
            float2 *__restrict__ bins, float *__restrict__ db, float scaledb)
{
	extern __shared__ float2 lds[];
	const unsigned int n = n1 * n2;
	float2 *a = lds, *b = lds + (size_t)n2 * rt;
	const size_t frame = blockIdx.y;
	const unsigned int row0 = blockIdx.x * rt;
	const float2 *win = work + frame * n;
	const unsigned int total = n2 * rt;
	/* global read is contiguous along n2 within a row; LDS layout is [n2][rt] */
	for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const unsigned int r = e / n2, i = e - r * n2;
		a[i * rt + r] = win[(size_t)(row0 + r) * n2 + i];
	}
	__syncthreads();
	const float2 *in = lds_fft(a, b, n2, rt, tw_sub, tw_sub_len / n2, threadIdx.x);
	for (unsigned int e = threadIdx.x; e < total; e += FFT_THREADS) {
		const unsigned int k2 = e / rt, r = e - k2 * rt;
		const unsigned int k = row0 + r + n1 * k2;
		const float2 v = in[e];
		if (bins)
			bins[frame * n + k] = v;
		if (db)
			db[frame * n + ((k + (n >> 1)) & (n - 1))] = to_db(v, scaledb);
	}
}

/* ------------------------------------------------------------------------------------
 * 65536-point fast path (BASELINE config 3): 256 x 256 four-step with the 256-point
 * sub-transforms done as 16 x 16 in REGISTERS -- each thread holds 16 points, does a
 * 16-point FFT, one exchange through LDS, another 16-point FFT.  One LDS round trip per
 * 256-point transform instead of eight (radix-2).
 * ------------------------------------------------------------------------------------ */

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

/* 16-point forward DFT in registers: decimation in frequency, then undo the bit reversal.
 * All indices are compile-time, so the loops dissolve into straight-line code and the
 * twiddles exp(-2*pi*i*j/len) into literals. */
__device__ __forceinline__ void fft16(float2 (&v)[16])
{
	const float c1 = 0.92387953251128673848f, s1 = 0.38268343236508978178f;   /* cos, sin(pi/8) */
	const float r2 = 0.70710678118654752440f;
	const float2 w16[8] = { {1.0f, 0.0f}, {c1, -s1}, {r2, -r2}, {s1, -c1},
	                        {0.0f, -1.0f}, {-s1, -c1}, {-r2, -r2}, {-c1, -s1} };
#pragma unroll
	for (int len = 16; len >= 2; len >>= 1) {
		const int half = len >> 1;
#pragma unroll
		for (int base = 0; base < 16; base += len) {
#pragma unroll
			for (int j = 0; j < half; ++j) {
				const float2 a = v[base + j], b = v[base + j + half];
				v[base + j] = cadd(a, b);
				const float2 d = csub(a, b);
				const int tw = j * (16 / len);             /* W_len^j = W_16^(j*16/len) */
				if (tw == 0)
					v[base + j + half] = d;
				else if (tw == 4)
					v[base + j + half] = make_float2(d.y, -d.x);          /* times -i */
				else
					v[base + j + half] = cmul(d, w16[tw]);
			}
		}
	}
	/* bit-reversed -> natural order (a register renaming) */
	float2 t;
#define SWAP16(a, b) t = v[a]; v[a] = v[b]; v[b] = t;
	SWAP16(1, 8) SWAP16(2, 4) SWAP16(3, 12) SWAP16(5, 10) SWAP16(7, 14) SWAP16(11, 13)
#undef SWAP16
}

/* W_256^m from the half-circle table (128 entries): W^(m+128) = -W^m */
__device__ __forceinline__ float2 w256(const float2 *__restrict__ tw, unsigned int m)
{
	const float2 w = tw[m & 127u];
	return (m & 128u) ? make_float2(-w.x, -w.y) : w;
}

typedef float nt_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 nt_load2(const float2 *p)
{
	const nt_v2f v = __builtin_nontemporal_load((const nt_v2f *)p);
	return make_float2(v.x, v.y);
}
__device__ __forceinline__ void nt_store2(float2 *p, float2 v)
{
	__builtin_nontemporal_store((nt_v2f){v.x, v.y}, (nt_v2f *)p);
}

/* write-through (sc1) stores: data that the NEXT launch reads (pass 1's intermediate) or nothing on the chip reads again
 * (the dB rows) leave the L2 as they are written, not at the end-of-kernel release.  r03, 121 frames on one box: pass 1
 * 25.6 -> 23.8 us, pass 2 16.9 -> 16.5 us (profiles/r03_fft_pass1_ablation.txt, section 4) */
__device__ __forceinline__ void wt_store2(float2 *p, float2 v)
{
	union { float2 f; unsigned long long u; } cv;
	cv.f = v;
	__hip_atomic_store((unsigned long long *)p, cv.u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wt_store1(float *p, float v)
{
	__hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define F256_S 272        /* LDS row stride (float2): 16 x 16 plus 16 -> conflict-free exchanges */

/* pass 1: 16 adjacent columns n2 of FPW consecutive frames; thread (t = tid >> 4, c = tid & 15).
 * grid = (16, ceil(frames / FPW)).  work[k1][n2] = W_65536^(n2*k1) * sum_n1 w[n]x[n] W_256^(n1*k1).
 * FPW = 1: one frame per workgroup (small batches: the launch must fill the chip).  FPW = 4 (batches from
 * FFT64K_P1_LONG_MIN frames on): the window values a thread needs are the same 16 for every frame and stay in registers, as do
 * the two twiddle tables in LDS; the next frame's loads are issued before this frame's arithmetic; and at the reference's own
 * hop of half a frame, rows 128..255 of a frame are rows 0..127 of the next -- this thread already holds them.
 * (r03, 121 frames on one box: 25.0 -> 23.0 us; profiles/r03_fft_pass1_ablation.txt section 5.) */
template <unsigned int FPW>
__global__ void __launch_bounds__(256)
k_fft64k_pass1(const float2 *__restrict__ iq, size_t hop, const float *__restrict__ window,
               const float *__restrict__ window_p1, const float2 *__restrict__ tw256, const float2 *__restrict__ tw_n, float2 *__restrict__ work,
               unsigned int frames)
{
	__shared__ float2 ex[16 * F256_S];
	/* Twiddles from two 256-entry tables in LDS, W_65536^m = W_256^(m >> 8) * W_65536^(m & 255): the
	 * 65536 inter-pass twiddles of a frame were one 8-byte gather each from a 256 KB table in L2 --
	 * as many memory instructions as the samples themselves, and the slower half of this kernel
	 * (r02 profile: 40.8 us for 121 frames, against 19.8 us for pass 2) */
	__shared__ float2 thi[256], tlo[256];
	thi[threadIdx.x] = w256(tw256, threadIdx.x);
	tlo[threadIdx.x] = tw_n[threadIdx.x];
	const unsigned int c = threadIdx.x & 15u, t = threadIdx.x >> 4;
	const unsigned int col = blockIdx.x * 16u + c;
	const unsigned int f0 = blockIdx.y * FPW;
	float wv[16];
	float2 nx[16];                                         /* the frame about to be transformed, as loaded */
	{
		const float2 *x = iq + (size_t)f0 * hop;
#pragma unroll
		for (int a = 0; a < 16; ++a)
			nx[a] = x[(a * 16u + t) * 256u + col];
		const float4 *wp = (const float4 *)window_p1 + (size_t)blockIdx.x * 1024u + threadIdx.x;   /* [tile][a / 4][thread] */
#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const float4 w4 = wp[q * 256u];
			wv[4 * q] = w4.x, wv[4 * q + 1] = w4.y, wv[4 * q + 2] = w4.z, wv[4 * q + 3] = w4.w;
		}
	}
#pragma unroll 1
	for (unsigned int fi = 0; fi < FPW; ++fi) {
		const unsigned int f = f0 + fi;
		if (f >= frames)
			break;
		float2 v[16];
#pragma unroll
		for (int a = 0; a < 16; ++a)
			v[a] = make_float2(nx[a].x * wv[a], nx[a].y * wv[a]);          /* spectrumsink.cxx:109-112 */
		if (FPW > 1 && fi + 1 < FPW && f + 1 < frames) {
			const float2 *xn = iq + (size_t)(f + 1) * hop;
			if (hop == 32768u) {
#pragma unroll
				for (int a = 0; a < 8; ++a)
					nx[a] = nx[a + 8];
#pragma unroll
				for (int a = 8; a < 16; ++a)
					nx[a] = xn[(a * 16u + t) * 256u + col];
			} else {
#pragma unroll
				for (int a = 0; a < 16; ++a)
					nx[a] = xn[(a * 16u + t) * 256u + col];
			}
		}
		fft16(v);                                          /* over a: k = 0..15, for n1 = a*16 + t */
		__syncthreads();                                   /* the tables; the frame before's reads of `ex` */
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const float2 w = thi[(t * k) & 255u];          /* W_256^(t*k) */
			ex[k * F256_S + t * 16u + c] = (k == 0) ? v[k] : cmul(v[k], w);
		}
		__syncthreads();
#pragma unroll
		for (int b = 0; b < 16; ++b)
			v[b] = ex[t * F256_S + b * 16u + c];           /* this thread now owns k_low = t */
		fft16(v);                                          /* over b: k1 = t + 16*k_high */
		float2 *wout = work + (size_t)f * 65536u;
#pragma unroll
		for (int kh = 0; kh < 16; ++kh) {
			const unsigned int k1 = t + 16u * kh;
			const unsigned int m = col * k1;               /* < 65536 */
			const float2 w = cmul(thi[m >> 8], tlo[m & 255u]);
			/* intermediate laid out [column tile][k1][16]: this workgroup's 32 KiB are one contiguous run,
			 * and a pass-2 workgroup (16 rows k1) reads 2 KiB runs from each of the 16 tiles */
			wt_store2(&wout[(blockIdx.x * 256u + k1) * 16u + c], cmul(v[kh], w));
		}
	}
}

/* window_p1 (host): thread (t, c) of column tile T above multiplies rows a*16 + t, a = 0..15, of column T*16 + c: stored as
 * [T][a / 4][thread][a % 4], a thread takes its 16 values with four 16-byte loads that are contiguous across the threads of
 * a wave (they were 16 four-byte loads in 64-byte runs: as many memory instructions as the samples) */
static std::vector<float> fft64k_window_p1(const std::vector<float> &win)
{
	std::vector<float> wp(65536);
	for (unsigned int T = 0; T < 16; ++T)
		for (unsigned int tid = 0; tid < 256; ++tid)
			for (unsigned int a = 0; a < 16; ++a)
				wp[((T * 4 + a / 4) * 256 + tid) * 4 + a % 4] = win[(a * 16 + (tid >> 4)) * 256 + T * 16 + (tid & 15)];
	return wp;
}

/* pass 2: 16 adjacent rows k1 of the intermediate; bins X[k1 + 256*k2].  Loads run with t
 * fastest (a row is contiguous), stores with the row index fastest (bins of neighbouring
 * k1 are contiguous).  grid = (16, frames). */
__global__ void __launch_bounds__(256)
k_fft64k_pass2(const float2 *__restrict__ work, const float2 *__restrict__ tw256,
               float2 *__restrict__ bins, float *__restrict__ db, float scaledb)
{
	__shared__ float2 ex[16 * 289];
	__shared__ float2 thi[256];
	thi[threadIdx.x] = w256(tw256, threadIdx.x);
	const unsigned int row0 = blockIdx.x * 16u;
	const float2 *win = work + (size_t)blockIdx.y * 65536u;
	float2 v[16];
	{
		const unsigned int t = threadIdx.x & 15u, r = threadIdx.x >> 4;
#pragma unroll
		for (int a = 0; a < 16; ++a)
			v[a] = win[(a * 256u + row0 + r) * 16u + t];   /* column a*16 + t of row row0 + r (tiled, see pass 1) */
		fft16(v);
		__syncthreads();                               /* the table */
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const float2 w = thi[(t * k) & 255u];
			ex[k * 289u + r * 17u + t] = (k == 0) ? v[k] : cmul(v[k], w);
		}
	}
	__syncthreads();
	{
		const unsigned int r = threadIdx.x & 15u, t = threadIdx.x >> 4;   /* t = k_low */
#pragma unroll
		for (int b = 0; b < 16; ++b)
			v[b] = ex[t * 289u + r * 17u + b];
		fft16(v);
		const size_t fbase = (size_t)blockIdx.y * 65536u;
#pragma unroll
		for (int kh = 0; kh < 16; ++kh) {
			const unsigned int k = row0 + r + 256u * (t + 16u * kh);
			if (bins)
				bins[fbase + k] = v[kh];
			if (db) {
				wt_store1(&db[fbase + ((k + 32768u) & 65535u)], to_db(v[kh], scaledb));
			}
		}
	}
}

/* getSpectrum on stored bins (io/spectrumsink.cxx:125-142) */
__global__ void k_bins_to_db(const float2 *__restrict__ bins, unsigned int n, float *__restrict__ db,
                             float scaledb)
{
	for (unsigned int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
		db[(k + (n >> 1)) & (n - 1)] = to_db(bins[k], scaledb);
}

/* a pixel column's value after dB value `d`, the i-th of the bins that map to it, with `v` so far */
__device__ __forceinline__ float waterfall_pick(float v, float d, unsigned int i, int hold)
{
	if (!isfinite(d))
		d = -10000.0f;                                            /* waterfallhandler.cxx:65-68 */
	return (i == 0 || !hold || d > v) ? d : v;                    /* last one wins, or running max */
}

/* waterfall.js:94-106, in double like JavaScript numbers */
__device__ __forceinline__ uint8_t waterfall_palette(float v)
{
	double c = floor(((double)v + 50.0) / 25.0 * 255.0);
	c = c < 0.0 ? 0.0 : (c > 255.0 ? 255.0 : c);
	return (uint8_t)c;
}

/* waterfall row: dB + fft-shift of the stored bins reduced to `width` pixel columns */
__global__ void k_waterfall_row(const float2 *__restrict__ bins, unsigned int n, unsigned int width, int hold,
                                float scaledb, float *__restrict__ db_row, uint8_t *__restrict__ palette)
{
	const unsigned int per = n / width;
	for (unsigned int x = blockIdx.x * blockDim.x + threadIdx.x; x < width; x += gridDim.x * blockDim.x) {
		float v = 0.0f;
		for (unsigned int i = 0; i < per; ++i) {
			const unsigned int shifted = x * per + i;                 /* index in the shifted row */
			const unsigned int k = (shifted + (n >> 1)) & (n - 1);     /* FFTW-order bin */
			v = waterfall_pick(v, to_db(bins[k], scaledb), i, hold);
		}
		if (db_row)
			db_row[x] = v;
		if (palette)
			palette[x] = waterfall_palette(v);
	}
}

/* the same reduction on `nrows` shifted dB rows of n floats (wr_spectrum_batch_avg's, wr_spectrum_batch_db's): a thread
 * per (row, pixel column), the rows' pixel rows back to back */
__global__ void k_rows_waterfall(const float *__restrict__ db, unsigned int n, size_t nrows, unsigned int width, int hold,
                                 float *__restrict__ db_rows, uint8_t *__restrict__ palette)
{
	const unsigned int per = n / width;
	const size_t total = nrows * width;
	for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
		const float *col = db + e * per;                           /* (row * n + x * per: width * per = n) */
		float v = 0.0f;
		for (unsigned int i = 0; i < per; ++i)
			v = waterfall_pick(v, col[i], i, hold);
		if (db_rows)
			db_rows[e] = v;
		if (palette)
			palette[e] = waterfall_palette(v);
	}
}

/* 10*log10f(x) - 20*log10f(N) of a power (to_db's expression behind its sum) */
__device__ __forceinline__ float power_to_db(float p, float scaledb)
{
	return 10.0f * log10f(p) - scaledb;
}

/* wr_spectrum_batch_avg's reduction over the frames of a chunk: bins[group][frame][n] of `groups` groups, `frames` of each.
 * One thread per (group, bin k): neighbouring threads load neighbouring bins of one frame.  Per frame the power
 * p = fl(fl(re*re) + fl(im*im)) (the library is built with -ffp-contract=off), sum = ((p_0 + p_1) + p_2) + ... in ONE float
 * in frame order, peak the largest p.  `first`: the chunk begins its groups' frames; else sum and peak continue from
 * carry[group][k] = (sum, peak), so a cut between two chunks leaves no trace in the bits.  `last`: mean = sum / nframes and
 * peak go out as they are (linear) or in dB, at the fft-shifted position; else (sum, peak) go to the carry. */
__global__ void __launch_bounds__(SPEC_REDUCE_THREADS)
k_spec_reduce(const float2 *__restrict__ bins, unsigned int n, size_t groups, size_t frames, int first, int last,
              float2 *__restrict__ carry, float nframes, int linear, float scaledb,
              float *__restrict__ mean, float *__restrict__ peak)
{
	const size_t e = (size_t)blockIdx.x * SPEC_REDUCE_THREADS + threadIdx.x;
	if (e >= groups * n)
		return;
	const size_t g = e / n;
	const unsigned int k = (unsigned int)(e - g * n);
	const float2 *b = bins + g * frames * n + k;
	float sum, top;
	size_t f = 0;
	if (first) {
		const float2 v = b[0];
		sum = top = v.x * v.x + v.y * v.y;
		f = 1;
	} else {
		const float2 c = carry[e];
		sum = c.x;
		top = c.y;
	}
	/* eight frames' loads in flight per thread: the adds wait for one another, the loads need not */
	for (; f + 8 <= frames; f += 8) {
		float2 v[8];
#pragma unroll
		for (int i = 0; i < 8; ++i)
			v[i] = b[(f + i) * n];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			const float p = v[i].x * v[i].x + v[i].y * v[i].y;
			sum = sum + p;
			top = p > top ? p : top;
		}
	}
	for (; f < frames; ++f) {
		const float2 v = b[f * n];
		const float p = v.x * v.x + v.y * v.y;
		sum = sum + p;
		top = p > top ? p : top;
	}
	if (!last) {
		carry[e] = make_float2(sum, top);
		return;
	}
	const float avg = sum / nframes;
	const size_t o = g * n + ((k + (n >> 1)) & (n - 1u));
	if (mean)
		mean[o] = linear ? avg : power_to_db(avg, scaledb);
	if (peak)
		peak[o] = linear ? top : power_to_db(top, scaledb);
}

hipError_t wrk_waterfall_row(hipStream_t st, const float *bins, unsigned int n, unsigned int width, int hold,
                             float *db_row, uint8_t *palette)
{
	const float scaledb = 20.0f * log10f((float)n);
	k_waterfall_row<<<grid_for(width, 256, FFT_WATERFALL_GRID_CAP), 256, 0, st>>>((const float2 *)bins, n, width, hold, scaledb,
	                                                                             db_row, palette);
	return hipGetLastError();
}

hipError_t wrk_rows_waterfall(hipStream_t st, const float *db, unsigned int n, size_t nrows, unsigned int width, int hold,
                              float *db_rows, uint8_t *palette)
{
	k_rows_waterfall<<<wrp_rows_waterfall_grid(nrows, width), 256, 0, st>>>(db, n, nrows, width, hold, db_rows, palette);
	return hipGetLastError();
}

hipError_t wrk_spec_reduce(hipStream_t st, const float *bins, unsigned int n, size_t groups, size_t frames, bool first, bool last,
                           float *carry, size_t nframes_fft, int linear, float *mean, float *peak)
{
	const float scaledb = 20.0f * log10f((float)n);
	k_spec_reduce<<<wrp_spec_reduce_grid(n, groups), SPEC_REDUCE_THREADS, 0, st>>>((const float2 *)bins, n, groups, frames, first, last,
	                                                                             (float2 *)carry, (float)nframes_fft, linear, scaledb,
	                                                                             mean, peak);
	return hipGetLastError();
}

hipError_t wrk_bins_to_db(hipStream_t st, const float *bins, unsigned int n, float *db)
{
	const float scaledb = 20.0f * log10f((float)n);
	k_bins_to_db<<<grid_for(n, 256, FFT_DB_GRID_CAP), 256, 0, st>>>((const float2 *)bins, n, db, scaledb);
	return hipGetLastError();
}

/* ---- the plan: the shape (wr_plan.h), the tables the kernels read, the work area between the passes ---- */

void wrk_fft_plan_free(WrFftPlan *P)
{
	(void)hipFree(P->tw_n);
	(void)hipFree(P->tw_sub);
	(void)hipFree(P->window);
	(void)hipFree(P->window_p1);
	(void)hipFree(P->work);
	memset(P, 0, sizeof(*P));
}

static hipError_t fft_table(float **dev, const std::vector<float> &host)
{
	hipError_t e = hipMalloc((void **)dev, host.size() * sizeof(float));
	if (e == hipSuccess)
		e = hipMemcpy(*dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
	return e;
}

hipError_t wrk_fft_plan_create(WrFftPlan *P, unsigned int n, unsigned int channels)
{
	memset(P, 0, sizeof(*P));
	P->n = n;
	P->channels = channels;
	P->shape = wrp_fft_shape(n, channels);
	const WrFftShape &S = P->shape;
	std::vector<float> tw(n), win(n), tws(S.sub ? S.sub : 2);
	wrd_twiddles(n, tw.data());
	wrd_spectrum_window(n, win.data());
	if (S.sub)
		wrd_twiddles(S.sub, tws.data());
	hipError_t e = fft_table(&P->tw_n, tw);
	if (e == hipSuccess)
		e = fft_table(&P->window, win);
	if (e == hipSuccess)
		e = fft_table(&P->tw_sub, tws);
	if (e == hipSuccess && S.path == WR_FFT_REG64K)
		e = fft_table(&P->window_p1, fft64k_window_p1(win));
	if (e == hipSuccess && S.path != WR_FFT_SINGLE) {
		/* one frame; wrk_fft_plan_reserve grows it */
		e = hipMalloc((void **)&P->work, (size_t)n * 2 * sizeof(float));
		if (e == hipSuccess)
			P->work_frames = 1;
	}
	if (e != hipSuccess)
		wrk_fft_plan_free(P);
	return e;
}

hipError_t wrk_fft_plan_reserve(WrFftPlan *P, size_t frames, wr_dev *dev)
{
	if (P->shape.path == WR_FFT_SINGLE)
		return hipSuccess;
	const size_t want = wrp_fft_work_frames(P->n, P->work_frames, frames);
	if (want == P->work_frames)
		return hipSuccess;
	hipError_t e = wrc_dev_stream_sync(dev);                /* (whatever still uses the old area) */
	if (e != hipSuccess)
		return e;
	(void)hipFree(P->work);
	P->work = nullptr;
	P->work_frames = 0;
	e = hipMalloc((void **)&P->work, want * P->n * 2 * sizeof(float));
	if (e == hipSuccess)
		P->work_frames = want;
	return e;
}

/* ---- the launches: a plan's numbers (wr_plan.h), what only the runtime can give (allow_lds), the launch ---- */

/* every kernel with dynamic LDS may be asked for the whole budget by some plan, and k_fft_pass2 serves plans of every size:
 * each instance is allowed FFT_LDS_MAX once per device, whatever the first call needs */
template <auto KERNEL>
static hipError_t fft_allow_lds(void)
{
	static bool done[WR_MAX_DEVICES];
	return allow_lds((const void *)KERNEL, FFT_LDS_MAX, done);
}

hipError_t wrk_fft_frames(hipStream_t st, const WrFftPlan &P, const float *iq, size_t hop,
                          size_t nframes_fft, float *bins_out, float *db_out)
{
	return wrk_fft_groups(st, P, iq, hop, nframes_fft, 1, 0, bins_out, db_out);
}

hipError_t wrk_fft_groups(hipStream_t st, const WrFftPlan &P, const float *iq, size_t hop, size_t nframes_fft, size_t ngroups,
                          size_t gstride, float *bins_out, float *db_out)
{
	if (!nframes_fft || !ngroups)
		return hipSuccess;
	const WrFftShape &S = P.shape;
	const float scaledb = 20.0f * log10f((float)P.n);   /* spectrumsink.cxx:127 */
	const float2 *tw_n = (const float2 *)P.tw_n, *tw_sub = (const float2 *)P.tw_sub;
	hipError_t e;
	if (S.path == WR_FFT_SINGLE) {
		/* every group's frames in one launch */
		const WrFftLaunch L = wrp_fft_launch(S, nframes_fft * ngroups);
		const unsigned int fpg = (unsigned int)nframes_fft;
		if ((e = S.real ? fft_allow_lds<k_fft_real_single>() : fft_allow_lds<k_fft_single>()) != hipSuccess)
			return e;
		if (S.real)
			k_fft_real_single<<<L.g1x, FFT_THREADS, L.lds1, st>>>(iq, hop, fpg, gstride, P.n, P.window, tw_n, (float2 *)bins_out,
			                                                      db_out, scaledb);
		else
			k_fft_single<<<L.g1x, FFT_THREADS, L.lds1, st>>>((const float2 *)iq, hop, fpg, gstride, P.n, P.window, tw_n,
			                                                 (float2 *)bins_out, db_out, scaledb);
		return hipGetLastError();
	}
	if (ngroups > 1) {
		/* the two-pass paths: a loop over the groups */
		for (size_t g = 0; g < ngroups; ++g) {
			const size_t row = g * nframes_fft * P.n;
			if ((e = wrk_fft_groups(st, P, iq + P.channels * g * gstride, hop, nframes_fft, 1, 0, bins_out ? bins_out + 2 * row : nullptr,
			                        db_out ? db_out + row : nullptr)) != hipSuccess)
				return e;
		}
		return hipSuccess;
	}
	if (S.path == WR_FFT_FOUR_STEP) {
		if ((e = S.real ? fft_allow_lds<k_fft_pass1<true>>() : fft_allow_lds<k_fft_pass1<false>>()) != hipSuccess)
			return e;
		if ((e = fft_allow_lds<k_fft_pass2>()) != hipSuccess)
			return e;
	}
	/* two launches per chunk of the work area (real: three -- pass 2 leaves the packed transform in the area's second half
	 * and k_fft_untangle makes the frame's bins of it) */
	float2 *work = (float2 *)P.work;
	float2 *zbuf = S.real ? work + wrp_fft_untangle_offset(P.work_frames, S.points) : nullptr;
	for (size_t done = 0; done < nframes_fft;) {
		const size_t batch = wrp_fft_chunk(nframes_fft - done, P.work_frames);
		const WrFftLaunch L = wrp_fft_launch(S, batch);
		const float2 *src = (const float2 *)(iq + P.channels * done * hop);
		float2 *bins = bins_out ? (float2 *)(bins_out + 2 * done * P.n) : (float2 *)nullptr;
		float *db = db_out ? db_out + done * P.n : (float *)nullptr;
		const dim3 g1(L.g1x, L.g1y), g2(L.g2x, L.g2y);
		if (S.path == WR_FFT_REG64K) {
			if (L.fpw == 4u)
				k_fft64k_pass1<4u><<<g1, 256, 0, st>>>(src, hop, P.window, P.window_p1, tw_sub, tw_n, work, (unsigned int)batch);
			else
				k_fft64k_pass1<1u><<<g1, 256, 0, st>>>(src, hop, P.window, P.window_p1, tw_sub, tw_n, work, (unsigned int)batch);
			k_fft64k_pass2<<<g2, 256, 0, st>>>(work, tw_sub, bins, db, scaledb);
		} else {
			if (S.real)
				k_fft_pass1<true><<<g1, FFT_THREADS, L.lds1, st>>>(src, hop, S.n1, S.n2, L.ct, P.window, tw_sub, S.sub, tw_n, work);
			else
				k_fft_pass1<false><<<g1, FFT_THREADS, L.lds1, st>>>(src, hop, S.n1, S.n2, L.ct, P.window, tw_sub, S.sub, tw_n, work);
			k_fft_pass2<<<g2, FFT_THREADS, L.lds2, st>>>(work, S.n1, S.n2, L.rt, tw_sub, S.sub, S.real ? zbuf : bins,
			                                             S.real ? (float *)nullptr : db, S.real ? 0.0f : scaledb);
			if (S.real)
				k_fft_untangle<<<dim3(L.g3x, L.g3y), FFT_THREADS, 0, st>>>(zbuf, P.n, tw_n, bins, db, scaledb);
		}
		if ((e = hipGetLastError()) != hipSuccess)
			return e;
		done += batch;
	}
	return hipSuccess;
}

hipError_t wrk_fft_cols(hipStream_t st, const WrFftPlan &P, const float *iq, unsigned int S, unsigned int cols, size_t first,
                        float *db, int num_cus)
{
	if (P.channels != 2 || P.shape.path != WR_FFT_SINGLE || P.n < 8 || P.n > FFT_LDS_POINTS || !cols || cols % 64u || cols > S)
		return hipErrorInvalidValue;
	const unsigned int ct = wrp_fft_cols_ct(P.n, cols, num_cus);
	const size_t lds = (size_t)2 * P.n * ct * sizeof(float2);
	hipError_t e = fft_allow_lds<k_fft_cols>();
	if (e != hipSuccess)
		return e;
	k_fft_cols<<<cols / ct, FFT_THREADS, lds, st>>>((const float2 *)iq, S, cols, first, P.n, ct, P.window, (const float2 *)P.tw_n, db,
	                                             20.0f * log10f((float)P.n));
	return hipGetLastError();
}
