/*
 * wr_detect.hip -- the band scan (wr_spectrum_rows_detect): the noise floor of every span of every row as an exact order
 * statistic, and the row's occupied segments as records.  The rule is include/webradio_amd.h's; integers decide, apart from
 * the one float operation (the threshold on the floor) and the one float compare (a bin against it).
 *
 * k_detect_floor: a workgroup of 256 threads is one span of one row.  Floats are ordered by their keys (det_key: a
 * monotone map onto unsigned integers under which NaNs lie outside [key(-inf), key(+inf)]), and the floor is found by a
 * radix select: four passes of eight bits, most significant first.  A pass counts, in a 256-bin histogram in LDS, the
 * digit of every key that matches the digits chosen so far; wave 0 scans the 256 counts and hands on the digit in which
 * the rank falls and the rank within it.  The first pass counts every non-NaN key, so its total is m.  A span of up to
 * DETECT_LDS_KEYS bins keeps its keys in LDS after the first pass; a larger one reads the row again (4 MB at most).
 * The values of a dB noise row share their top bits: lanes of a wave that hold the same digit are found with eight
 * ballots and the lowest of them adds their number, so a wave issues one atomic per distinct digit, not 64 on one address.
 *
 * k_detect_segments: a workgroup of 256 threads is one row, walked in tiles of 1024 bins, 4 consecutive bins a thread.
 * A tile in which no wave finds a hot bin (a ballot a wave, one barrier) is done.  Otherwise three forward scans, each a
 * thread's own bins in order, then __shfl_up over the wave's thread totals, then the wave totals through LDS (as k_agc_rows
 * does its prefix maximum):
 *   1. the last hot bin in front of each bin (prefix maximum) -- from it, which hot bins start a segment;
 *   2. the open segment in front of each bin: first, hot, and the maximum of key << 32 | ~index (segmented by the starts);
 *   3. the number of kept segments closed in front of each bin (prefix sum) -- where a record goes.
 * A segment is closed by the thread that starts the next one; the last one by the end of the window.  What a tile hands
 * to the next: the last hot bin, the open segment, the kept count.  A tile without a hot bin changes none of them.
 * One workgroup walks its row's tiles one after the other, so the row's values and floors are loaded eight tiles ahead.
 */
#include "wr_internal.h"

#define DET_KEY_LO 0x007fffffu                  /* det_key(-inf) */
#define DET_KEY_HI 0xff800000u                  /* det_key(+inf) */
#define DET_NAN    0x7fc00000u
#define DET_AHEAD  4u                           /* tiles of k_detect_segments whose loads are in flight together; even */
#define DET_LOADS  8u                           /* keys of a thread in flight per trip of k_detect_floor's counting loop */

static_assert(DETECT_THREADS == 256u, "k_detect_floor: a thread per histogram bin");
static_assert(DETECT_WAVES * WR_LANES == DETECT_THREADS, "whole waves");

__device__ __forceinline__ unsigned int det_key(unsigned int u)
{
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned int det_unkey(unsigned int k)
{
	return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
}

/* floors[item] for item = row * nspans + span index; dynamic LDS: WrDetectPlan::lds_floor */
__global__ void __launch_bounds__(DETECT_THREADS)
k_detect_floor(const float *__restrict__ rows, unsigned int n, unsigned int bin0, unsigned int span, unsigned int nspans,
               unsigned int percent, int keys_in_lds, float *__restrict__ floors)
{
	extern __shared__ unsigned int det_lds[];
	unsigned int *hist = det_lds, *sel = det_lds + 256, *keys = det_lds + DETECT_FLOOR_HEAD;
	const unsigned int tid = threadIdx.x, lane = tid & (WR_LANES - 1u), w = tid / WR_LANES;
	const size_t item = blockIdx.x, r = item / nspans;
	const unsigned int j = (unsigned int)(item % nspans);
	const unsigned int *src = (const unsigned int *)(rows + r * n + bin0 + (size_t)j * span);
	unsigned int prefix = 0, mask = 0, rank = 0;
	for (unsigned int pass = 0; pass < 4u; ++pass) {
		const unsigned int shift = 24u - 8u * pass;
		const bool from_lds = keys_in_lds && pass > 0;
		hist[tid] = 0;
		__syncthreads();
		for (unsigned int i0 = 0; i0 < span; i0 += DETECT_THREADS * DET_LOADS) {
			unsigned int k[DET_LOADS];
#pragma unroll
			for (unsigned int u = 0; u < DET_LOADS; ++u) {
				const unsigned int i = i0 + u * DETECT_THREADS + tid;
				k[u] = i >= span ? 0u : from_lds ? keys[i] : det_key(src[i]);    /* (key 0 is a NaN's: never counted) */
				if (keys_in_lds && pass == 0 && i < span)
					keys[i] = k[u];
			}
#pragma unroll
			for (unsigned int u = 0; u < DET_LOADS; ++u) {
				if (i0 + u * DETECT_THREADS >= span)
					break;                                      /* (the same for every thread) */
				const bool take = k[u] >= DET_KEY_LO && k[u] <= DET_KEY_HI && (k[u] & mask) == prefix;
				const unsigned int digit = (k[u] >> shift) & 255u;
				unsigned long long peers = __ballot(take);      /* the lanes that count the same digit as this one */
#pragma unroll
				for (unsigned int b = 0; b < 8u; ++b) {
					const bool bit = (digit >> b) & 1u;
					const unsigned long long has = __ballot(bit);
					peers &= bit ? has : ~has;
				}
				if (take && lane == (unsigned int)__ffsll(peers) - 1u)
					atomicAdd(&hist[digit], (unsigned int)__popcll(peers));
			}
		}
		__syncthreads();
		if (w == 0) {
			/* lane l: counts 4 l .. 4 l + 3; an inclusive prefix sum over the lanes' sums */
			unsigned int c[4], sum = 0;
#pragma unroll
			for (unsigned int q = 0; q < 4u; ++q) {
				c[q] = hist[4u * lane + q];
				sum += c[q];
			}
			unsigned int inc = sum;
#pragma unroll
			for (unsigned int d = 1; d < WR_LANES; d <<= 1) {
				const unsigned int o = __shfl_up(inc, d);
				if (lane >= d)
					inc += o;
			}
			if (pass == 0) {
				const unsigned int m = __shfl(inc, WR_LANES - 1u);
				rank = m ? (unsigned int)(((unsigned long long)(m - 1u) * percent) / 100u) : 0u;
				if (lane == 0)
					sel[2] = m;
			}
			unsigned int below = inc - sum;                     /* keys in the digits in front of this lane's */
			if (below <= rank && rank < inc) {
#pragma unroll
				for (unsigned int q = 0; q < 4u; ++q) {
					if (rank >= below && rank < below + c[q]) {
						sel[0] = 4u * lane + q;
						sel[1] = rank - below;
					}
					below += c[q];
				}
			}
		}
		__syncthreads();
		if (sel[2] == 0) {
			/* nothing but NaNs */
			if (tid == 0)
				floors[item] = __uint_as_float(DET_NAN);
			return;
		}
		prefix |= sel[0] << shift;
		mask |= 255u << shift;
		rank = sel[1];
	}
	if (tid == 0)
		floors[item] = __uint_as_float(det_unkey(prefix));
}

/* ---- the three scans of k_detect_segments: what is scanned, its neutral element, a then b, a lane's value from d lanes down ---- */

struct DetMax {                                 /* a bin index + 1, 0: none */
	unsigned int v;
	static __device__ __forceinline__ DetMax none() { return {0u}; }
	static __device__ __forceinline__ DetMax join(DetMax a, DetMax b) { return {a.v > b.v ? a.v : b.v}; }
	static __device__ __forceinline__ DetMax up(DetMax a, unsigned int d) { return {__shfl_up(a.v, d)}; }
};

struct DetSum {
	unsigned int v;
	static __device__ __forceinline__ DetSum none() { return {0u}; }
	static __device__ __forceinline__ DetSum join(DetSum a, DetSum b) { return {a.v + b.v}; }
	static __device__ __forceinline__ DetSum up(DetSum a, unsigned int d) { return {__shfl_up(a.v, d)}; }
};

/* a run of bins as the open segment behind it sees it: `flag`: a segment starts inside the run, at `first`; `hot` and `peak`
 * (key << 32 | ~index, 0: none) count from that start, or over the whole run where there is none */
struct DetSeg {
	unsigned int flag, first, hot;
	unsigned long long peak;
	static __device__ __forceinline__ DetSeg none() { return {0u, 0u, 0u, 0ull}; }
	static __device__ __forceinline__ DetSeg join(DetSeg a, DetSeg b)
	{
		if (b.flag)
			return b;
		return {a.flag, a.first, a.hot + b.hot, a.peak > b.peak ? a.peak : b.peak};
	}
	static __device__ __forceinline__ DetSeg up(DetSeg a, unsigned int d)
	{
		return {__shfl_up(a.flag, d), __shfl_up(a.first, d), __shfl_up(a.hot, d), __shfl_up(a.peak, d)};
	}
};

/* the join of the values of every thread of the workgroup in front of this one, and of all of them; one barrier */
template <class T>
__device__ __forceinline__ T det_scan(T mine, T *wave_totals, T *all, unsigned int lane, unsigned int w)
{
	T inc = mine;
#pragma unroll
	for (unsigned int d = 1; d < WR_LANES; d <<= 1) {
		const T o = T::up(inc, d);
		if (lane >= d)
			inc = T::join(o, inc);
	}
	T before = T::up(inc, 1u);
	if (lane == 0)
		before = T::none();
	if (lane == WR_LANES - 1u)
		wave_totals[w] = inc;
	__syncthreads();
	T front = T::none(), total = T::none();
#pragma unroll
	for (unsigned int u = 0; u < DETECT_WAVES; ++u) {
		const T t = wave_totals[u];
		if (u < w)
			front = T::join(front, t);
		total = T::join(total, t);
	}
	*all = total;
	return T::join(front, before);
}

struct DetRule {
	unsigned int bin0, nbins, span, nspans, max_gap, min_width;
	float threshold;
	int linear;
};

__device__ __forceinline__ void det_store(wr_detection *out, unsigned int first, unsigned int last, unsigned int hot,
                                          unsigned long long peak, const float *floors, const DetRule &R)
{
	const unsigned int peak_bin = ~(unsigned int)peak;
	out->first = first;
	out->last = last;
	out->peak_bin = peak_bin;
	out->hot = hot;
	out->peak = __uint_as_float(det_unkey((unsigned int)(peak >> 32)));
	out->floor = floors[(peak_bin - R.bin0) / R.span];
}

/* the DETECT_PER bins of the window from bin k0 (a multiple of DETECT_PER) on and the floors of their spans; behind the
 * window: 0 and NaN, so that nothing there is hot.  Every load is issued whatever k0 is, from a clamped address: loads
 * under a branch would make the compiler wait for ALL loads in flight where a tile's values are first used, the tiles
 * ahead included. */
__device__ __forceinline__ void det_load(const float *__restrict__ win, const float *__restrict__ floors, const DetRule &R,
                                         unsigned int k0, float (&v)[DETECT_PER], float (&fl)[DETECT_PER])
{
	/* (one division: a span is 8 bins or more, so the thread's bins lie in one span or in two) */
	const unsigned int j = k0 / R.span, room = R.span - (k0 - j * R.span);
#pragma unroll
	for (unsigned int i = 0; i < DETECT_PER; ++i) {
		const bool in = k0 + i < R.nbins;
		const unsigned int js = i < room ? j : j + 1u;
		const float x = win[in ? k0 + i : R.nbins - 1u];
		const float f = floors[js < R.nspans ? js : R.nspans - 1u];
		v[i] = in ? x : 0.0f;
		fl[i] = in ? f : __uint_as_float(DET_NAN);
	}
}

/* floors: [rows][nspans]; det: [rows][max_det] or NULL with max_det = 0; count: [rows] */
__global__ void __launch_bounds__(DETECT_THREADS)
k_detect_segments(const float *__restrict__ rows, unsigned int n, DetRule R, const float *__restrict__ floors_all,
                  unsigned int max_det, wr_detection *__restrict__ det, unsigned int *__restrict__ count)
{
	__shared__ unsigned int wt_any[2][DETECT_WAVES];        /* two sets taken in turn: a tile without a hot bin has this one barrier */
	__shared__ DetMax wt_last[DETECT_WAVES];
	__shared__ DetSeg wt_seg[DETECT_WAVES];
	__shared__ DetSum wt_kept[DETECT_WAVES];
	static_assert(sizeof(wt_any) + sizeof(wt_last) + sizeof(wt_seg) + sizeof(wt_kept) == DETECT_SEG_LDS, "wr_plan.h: DETECT_SEG_LDS");
	const size_t r = blockIdx.x;
	const unsigned int lane = threadIdx.x & (WR_LANES - 1u), w = threadIdx.x / WR_LANES;
	const unsigned int j0 = threadIdx.x * DETECT_PER;               /* the thread's first bin of a tile */
	const float *win = rows + r * n + R.bin0;
	const float *floors = floors_all + r * R.nspans;
	wr_detection *out = det + r * max_det;
	unsigned int carry_last = 0;                                    /* the last hot bin so far, + 1 */
	DetSeg open = DetSeg::none();                                   /* the segment it belongs to */
	unsigned int kept = 0;                                          /* kept segments closed so far */
	/* the loads of DET_AHEAD tiles are in flight together, and those of the next DET_AHEAD behind them: alone, a tile's load
	 * and its floors' are two thirds of the tile's time */
	float vn[DET_AHEAD][DETECT_PER], fn[DET_AHEAD][DETECT_PER];
#pragma unroll
	for (unsigned int q = 0; q < DET_AHEAD; ++q)
		det_load(win, floors, R, q * DETECT_TILE + j0, vn[q], fn[q]);
	for (unsigned int base0 = 0; base0 < R.nbins; base0 += DET_AHEAD * DETECT_TILE) {
		float va[DET_AHEAD][DETECT_PER], fa[DET_AHEAD][DETECT_PER];
#pragma unroll
		for (unsigned int q = 0; q < DET_AHEAD; ++q) {
#pragma unroll
			for (unsigned int i = 0; i < DETECT_PER; ++i) {
				va[q][i] = vn[q][i];
				fa[q][i] = fn[q][i];
			}
			det_load(win, floors, R, base0 + (DET_AHEAD + q) * DETECT_TILE + j0, vn[q], fn[q]);
		}
#pragma unroll
		for (unsigned int q = 0; q < DET_AHEAD; ++q) {
			const unsigned int base = base0 + q * DETECT_TILE, set = q & 1u;
			if (base >= R.nbins)
				break;                                                  /* (every thread alike) */
			const float (&v)[DETECT_PER] = va[q];
			bool hot[DETECT_PER];
			DetMax mine_last = DetMax::none();
#pragma unroll
			for (unsigned int i = 0; i < DETECT_PER; ++i) {
				const float t = R.linear ? fa[q][i] * R.threshold : fa[q][i] + R.threshold;
				hot[i] = v[i] >= t;                                     /* (behind the window the floor is NaN) */
				if (hot[i])
					mine_last.v = R.bin0 + base + j0 + i + 1u;
			}
			/* a tile without a hot bin -- most tiles of a band -- costs a ballot and a barrier, no scan */
			const unsigned long long any = __ballot(mine_last.v != 0);
			if (lane == 0)
				wt_any[set][w] = any != 0;
			__syncthreads();
			unsigned int tile_any = 0;
#pragma unroll
			for (unsigned int u = 0; u < DETECT_WAVES; ++u)
				tile_any |= wt_any[set][u];
			if (!tile_any)
				continue;                                               /* (every thread alike) */
			/* 1. the last hot bin in front of the thread's bins */
			DetMax tile_last;
			unsigned int run = det_scan(mine_last, wt_last, &tile_last, lane, w).v;
			if (carry_last > run)
				run = carry_last;
			bool start[DETECT_PER];
			unsigned int prev[DETECT_PER];
			DetSeg mine_seg = DetSeg::none();
#pragma unroll
			for (unsigned int i = 0; i < DETECT_PER; ++i) {
				start[i] = false;
				prev[i] = run;
				if (hot[i]) {
					const unsigned int k = R.bin0 + base + j0 + i;
					start[i] = !run || k - run > R.max_gap;             /* k - (run - 1) - 1 cold bins between them */
					run = k + 1u;
					const DetSeg e = {start[i] ? 1u : 0u, start[i] ? k : 0u, 1u,
					                  (unsigned long long)det_key(__float_as_uint(v[i])) << 32 | (unsigned int)~k};
					mine_seg = DetSeg::join(mine_seg, e);
				}
			}
			/* 2. the open segment in front of the thread's bins */
			DetSeg tile_seg;
			DetSeg st = DetSeg::join(open, det_scan(mine_seg, wt_seg, &tile_seg, lane, w));
			unsigned int c_first[DETECT_PER], c_hot[DETECT_PER];
			unsigned long long c_peak[DETECT_PER];
			bool c_kept[DETECT_PER];
			DetSum mine_kept = DetSum::none();
#pragma unroll
			for (unsigned int i = 0; i < DETECT_PER; ++i) {
				c_kept[i] = false;
				c_first[i] = c_hot[i] = 0;
				c_peak[i] = 0;
				if (hot[i]) {
					const unsigned int k = R.bin0 + base + j0 + i;
					const DetSeg e = {start[i] ? 1u : 0u, start[i] ? k : 0u, 1u,
					                  (unsigned long long)det_key(__float_as_uint(v[i])) << 32 | (unsigned int)~k};
					if (start[i] && prev[i]) {
						/* this bin closes the segment [st.first, prev - 1] */
						c_kept[i] = prev[i] - st.first >= R.min_width;
						c_first[i] = st.first;
						c_hot[i] = st.hot;
						c_peak[i] = st.peak;
						mine_kept.v += c_kept[i] ? 1u : 0u;
					}
					st = DetSeg::join(st, e);
				}
			}
			/* 3. where the records go */
			DetSum tile_kept;
			unsigned int at = kept + det_scan(mine_kept, wt_kept, &tile_kept, lane, w).v;
#pragma unroll
			for (unsigned int i = 0; i < DETECT_PER; ++i) {
				if (c_kept[i]) {
					if (at < max_det)
						det_store(out + at, c_first[i], prev[i] - 1u, c_hot[i], c_peak[i], floors, R);
					++at;
				}
			}
			carry_last = tile_last.v;                                   /* (bins ascend: the tile's last hot bin is the row's) */
			open = DetSeg::join(open, tile_seg);
			kept += tile_kept.v;
		}
	}
	if (threadIdx.x == 0) {
		if (carry_last && carry_last - open.first >= R.min_width) {
			if (kept < max_det)
				det_store(out + kept, open.first, carry_last - 1u, open.hot, open.peak, floors, R);
			++kept;
		}
		count[r] = kept;
	}
}

hipError_t wrk_detect_rows(hipStream_t st, const float *rows, unsigned int n, size_t nrows, const wr_detect_rule *rule,
                           const WrDetectPlan &plan, unsigned int max_det, wr_detection *det, unsigned int *count, float *floors)
{
	if (!nrows)
		return hipSuccess;
	if (!rows || !rule || !count || !floors || (max_det && !det) || nrows > plan.chunk_rows || plan.lds_floor > DETECT_WG_LDS_MAX)
		return hipErrorInvalidValue;
	const DetRule R = {rule->bin0, rule->nbins, rule->span, plan.nspans, rule->max_gap, rule->min_width, rule->threshold,
	                   rule->linear};
	k_detect_floor<<<wrp_detect_floor_grid(plan, nrows), DETECT_THREADS, plan.lds_floor, st>>>(
		rows, n, rule->bin0, rule->span, plan.nspans, rule->percent, plan.keys_in_lds ? 1 : 0, floors);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return e;
	k_detect_segments<<<wrp_detect_segments_grid(nrows), DETECT_THREADS, 0, st>>>(rows, n, R, floors, max_det, det, count);
	return hipGetLastError();
}
