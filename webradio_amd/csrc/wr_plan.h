/*
 * wr_plan.h -- the launch geometry of every tuner launch (the per-block DDC, the long-filter DDC, the post stage, the audio
 * filter, the streaming launch), of the spectrum launches (the transform's shape and path, its passes' tiles, grids and
 * LDS, the work area and its chunks, the columns per workgroup of the channel spectra, the chunks, scratch cap and launch count
 * of the averaged spectra, the band scan's limits, grids, LDS and chunks of rows), of the voice bank and of the row kernels
 * (tone bank: chunks, grid and the cut of a push into its two summed stretches; DCS bank: the start of a push and its cut
 * into launches; resampler: the limits on L / M / P, the output frames, grid and input span of a push; levels: groups, grids,
 * LDS and the work area's layout; AGC: tile): which kernel instance, how many
 * workgroups per role, how much LDS, the group map, kslow, kmax, the post stage's runs of tiles.  The arithmetic alone, with
 * no HIP call and no environment read, so that a CPU test can hold it to the rule (tests/test_launch_plan.py through
 * tests/cxx/cpu_host_checks.cxx; tests/cxx/plan_sweeps.cxx sweeps it under the host compiler's sanitizers).  The launch
 * functions (wr_kernels.hip, wr_stream_kernel.inc, wr_fft.hip, the row kernels' files) obtain a plan,
 * ask the runtime for what only it can give (allow_lds, the occupancy query), and launch with the plan's numbers.  The only
 * home of the constants geometry depends on: the kernels use the same names.  Plain C++11.
 */
#ifndef WR_PLAN_H_
#define WR_PLAN_H_

#include <stddef.h>

#include "webradio_amd.h"

/* what a kernel calls too (WRP_HD): inlined into it by force, and a plain inline function for the host compiler */
#ifdef __HIPCC__
#define WRP_HD __host__ __device__ __forceinline__
#else
#define WRP_HD static inline
#endif

#define WR_LANES     64                    /* wavefront width on gfx950 */
#define WR_HIST      (WR_FIR_LENGTH - 1)   /* 63 frames of FIR history, lowpass.cxx:133 */
#define WR_SPLIT_N   256                   /* entries of the coarse and of the fine NCO table */
#define WR_TAPSETS   4                     /* distinct channel filters a lane group may mix in the fast DDC kernel:
                                              receivers of one tuner mostly share a passband (radio.cxx:78-79),
                                              the UI lets each choose its own (receiverhandler.cxx:130-137) */
#define WR_CU_LDS_BYTES (160u * 1024u)     /* LDS of one CU (gfx950) */

/* ---- the post stage (post_role, k_tuner_post) ---- */
#define POST_TK 16u                        /* audio frames per tile */
#define POST_THREADS 512u

/* ---- k_tuner_ddc.  LDS plan: [0, 128 KiB) the two replicated NCO tables (SPLIT only),
 * then one private 2 x 512 B sample window per wave (double buffered across units). ---- */
#define DDC_TABLE_BYTES   (2u * WR_SPLIT_N * 32u * 8u)
#define DDC_WAVES         16u
#define DDC_ROTATE_WAVES      8u          /* every ROTATE variant (folded or per-lane taps): 8-wave workgroups, */
#define DDC_ROTATE_WGS_PER_CU 4u          /* four per CU */
#define DDC_LDS_BYTES     (DDC_TABLE_BYTES + DDC_WAVES * 2u * 512u)
#define DDC_NG2_WAVES_PER_EU 6u           /* NG = 2 (two lane groups per wave, k_tuner_ddc): 80 registers, 6 waves per SIMD */

/* ---- k_tuner_ddc_long_rot ---- */
#define LONG_ROT_WAVES 8u
#define LONG_ROT_LDS   ((2u * WR_SPLIT_N + LONG_ROT_WAVES * 2u * 64u) * 8u + LONG_ROT_WAVES * 64u * 4u)

/* ---- k_tuner_audio ---- */
#define AUD_ROWS 352u          /* staged demod rows: 352 x 64 x 4 B = 88 KiB */
#define AUD_TMAX 16u
#define AUD_THREADS 1024u

/* ---- k_tuner_stream: the audio filter lengths a launch is built for, by audio decimation: 64 and 128 taps at every one,
 * 256 taps up to D2 = 3 -- from D2 = 4 on a 256-tap window is 85 KB and more, ONE workgroup per CU, and a launch needs two (a
 * DDC and a post workgroup: wrp_stream_roles): those tuners keep their launch per block, and no kernel is built for them. */
#define STREAM_NSEG4_MAX_D2 3u

static inline unsigned int grid_for(size_t n, unsigned int block, unsigned int cap)
{
	size_t g = (n + block - 1) / block;
	if (g < 1)
		g = 1;
	if (g > cap)
		g = cap;
	return (unsigned int)g;
}

/* ---- the group map: which lane groups a DDC launch works on, eight bits per entry, sixteen entries ---- */
struct WrGroupMap {
	unsigned long long gmap[2];
	unsigned int ngroups;                  /* entries in use, 16 at most */
	unsigned long long rest;               /* bit g: selected group g is beyond the 16 one launch maps */
};

/* `gsel`: bit g set = lane group g takes part (0 = all `slots_used / 64` of them, <= 64: wr_tuner_create caps max_channels) */
static inline WrGroupMap wrp_group_map(unsigned int slots_used, unsigned long long gsel)
{
	WrGroupMap m = {{0, 0}, 0, 0};
	const unsigned int allgroups = slots_used / 64u;
	for (unsigned int g = 0; g < allgroups; ++g)
		if (!gsel || ((gsel >> g) & 1ull)) {
			if (m.ngroups < 16u) {
				m.gmap[m.ngroups >> 3] |= (unsigned long long)g << ((m.ngroups & 7u) * 8u);
				++m.ngroups;
			} else {
				m.rest |= 1ull << g;
			}
		}
	return m;
}

/* the lane group of entry i < ngroups */
static inline unsigned int wrp_group_at(const WrGroupMap &m, unsigned int i)
{
	return (unsigned int)((m.gmap[i >> 3] >> ((i & 7u) * 8u)) & 255u);
}

/* output frames of a block whose window reaches into the block before: the first ceil(63 / D1), k1 at most (a block
 * without an output frame has none, whatever d1) */
static inline unsigned int wrp_kslow(unsigned int d1, size_t k1)
{
	if (!k1 || !d1)
		return 0;
	const unsigned int kslow = (WR_HIST + d1 - 1u) / d1;
	return kslow > k1 ? (unsigned int)k1 : kslow;
}

/* tap sets in a launch: the largest count among the lane groups it maps (`nsets`: WrTunerLaunch::nsets) */
static inline unsigned int wrp_kmax(const WrGroupMap &m, const unsigned char *nsets)
{
	unsigned int kmax = 1;
	for (unsigned int i = 0; i < m.ngroups; ++i) {
		const unsigned int g = wrp_group_at(m, i);
		if (g < 64u && nsets[g] > kmax)
			kmax = nsets[g];
	}
	return kmax;
}

/* ---- The audio decimations the post stage is built for (anything else takes the two-kernel path): 1..6, and 8 and 10 --
 * 256 k -> 32 k (BASELINE config 1), 240 k -> 24 k, 480 k -> 48 k.  with_post_d2 (wr_kernels.hip) instantiates these. ---- */
#define WR_POST_D2_LIST 1, 2, 3, 4, 5, 6, 8, 10

static inline bool wrp_post_d2_supported(unsigned int d2)
{
	static const unsigned int list[] = {WR_POST_D2_LIST};
	for (size_t i = 0; i < sizeof(list) / sizeof(list[0]); ++i)
		if (list[i] == d2)
			return true;
	return false;
}

/* LDS of a post-stage workgroup (post_role): the staged rows of (POST_TK - 1) d2 + 64 nseg frames, the tile, the modes */
static inline size_t post_lds_bytes(unsigned int d2, unsigned int nseg)
{
	return (((size_t)(POST_TK - 1u) * d2 + WR_FIR_LENGTH * nseg) * 64u + POST_TK * 65u + 64u) * sizeof(float);
}

/* ---- post tiling: a lane group's `tiles` tiles of POST_TK audio frames go to workgroups in runs of `run` consecutive
 * tiles, `ntiles` = ceil(tiles / run) workgroups per lane group.  Three rules. ---- */
struct WrPostTiling {
	unsigned int run, ntiles;
};

static inline unsigned int wrp_post_tiles(size_t k2)
{
	return (unsigned int)((k2 + POST_TK - 1) / POST_TK);
}

static inline WrPostTiling wrp_post_tiling(unsigned int tiles, unsigned int run)
{
	const WrPostTiling t = {run, (tiles + run - 1u) / run};
	return t;
}

/* riding in a DDC launch (wrk_post_args): as long a run as still leaves every CU a few workgroups */
static inline WrPostTiling wrp_post_tiling_riding(unsigned int tiles, unsigned int groups)
{
	const unsigned int all = tiles * groups;
	/* measured at C2 (500 tiles a block), us per block: 1 block per launch, run 1 / 2 / 4:
	 * 38.3 / 37.1 / 38.0; 4 blocks per launch: 33.6 / 32.3 / 32.2 */
	return wrp_post_tiling(tiles, all >= 1536u ? 4u : all >= 384u ? 2u : 1u);
}

/* on its own (wrk_tuner_post_args) the post stage has the chip to itself and is a chain of latencies: one tile per
 * workgroup, all of them in flight at once (runs of tiles are for the workgroups that ride in a
 * DDC launch, where instructions are what is short); 15.4 against 18.2 us for a C2 block */
static inline WrPostTiling wrp_post_tiling_alone(unsigned int tiles, unsigned int groups, unsigned int nseg)
{
	/* ... unless there are tiles enough to fill the chip several times over anyway (the flush behind a launch of
	 * several blocks): runs of tiles then save the rows two neighbouring tiles share from being loaded and
	 * demodulated twice (59 of 139 at D2 = 5) */
	const unsigned int all = tiles * groups;
	unsigned int run = all >= 4096u ? 2u : 1u;   /* C2, four blocks: 43.6 / 33.6 / 36.0 us at runs of 1 / 2 / 4 */
	if (nseg == 4u && all >= 384u)
		run = 2u;       /* 256 taps: a tile stages 331 rows for its 80 new ones (D2 = 5) and one workgroup fits a CU --
		                   C2 (500 tiles), us per block all in at runs of 1 / 2 / 4: 93 / 83 / 104 (128 taps: 62 / 69 / 79),
		                   profiles/r05_long_filter.txt */
	return wrp_post_tiling(tiles, run);
}

/* post-stage tiles per workgroup for a launch that may keep `max_post` post workgroups resident */
static inline unsigned int stream_post_run(unsigned int tiles, unsigned int groups, unsigned int max_post)
{
	unsigned int run = 1;
	while (run < tiles && ((tiles + run - 1u) / run) * groups > max_post)
		++run;
	return run;
}

/* the streaming launch (wrk_tuner_stream), for the `n_post` post workgroups it keeps resident */
struct WrStreamTiling {
	unsigned int min_run;                  /* the shortest runs that give every task a workgroup of its own */
	unsigned int run, ntiles;              /* what a block goes in while the host is ahead */
	unsigned int drain_run, drain_ntiles;  /* ... and a host-paced stream's blocks, and a closed stream's last ones */
	bool long_runs;                        /* `run` started from tasks for half the post workgroups, not from min_run */
	unsigned int widened;                  /* tiles the small-block rule then added to it */
};

static inline WrStreamTiling wrp_post_tiling_stream(unsigned int tiles, unsigned int groups, unsigned int n_post)
{
	WrStreamTiling t;
	/* (r06) tasks for HALF the post workgroups, not for all of them: a run's first tile demodulates its 59 rows of overlap a
	 * second time and reads them a second time, and the launch runs at the package's power limit -- what a block costs is what
	 * it spends (profiles/r06_power.txt).  C2: runs of 5 tiles (100 tasks a block, 1.15 x the rows) instead of 2 (252, 1.37 x):
	 * 27.9-28.0 against 29.7 us per block; consecutive blocks' tasks go round the post workgroups (stream_post's `rot`), so two
	 * blocks' post stages are in flight side by side.  Longer still (8: 28.6, 12: the post stage no longer keeps up) loses. */
	t.min_run = stream_post_run(tiles, groups, n_post);
	t.run = t.min_run;
	t.long_runs = t.min_run >= 2u && n_post >= 8u;          /* (a block with more tiles than post workgroups: the throughput case) */
	if (t.long_runs)
		t.run = stream_post_run(tiles, groups, n_post / 2u);
	/* (r06) small blocks: fewer, longer tasks -- up to four tiles each, down to a quarter of the post workgroups per block --
	 * so that the post stages of up to four consecutive blocks are in flight on different workgroups (stream_post's `rot`):
	 * a task's time is latency, and a 64 ms block of BASELINE config 1 is 128 tiles */
	t.widened = 0;
	while (t.run < 4u && t.run < tiles && ((tiles + t.run - 1u) / t.run) * groups > n_post / 4u &&
	       ((tiles + t.run - 1u) / t.run) * groups <= n_post / 2u) {
		++t.run;
		++t.widened;
	}
	t.ntiles = (tiles + t.run - 1u) / t.run;
	/* the stream's last blocks (tasks by ticket, the DDC workgroups helping): the shortest runs -- what ends a closed stream is
	 * the latency of its last tasks (secondary.frontend's launch-per-block mode: 123 against 134 us with the long runs) */
	t.drain_run = t.min_run < t.run ? t.min_run : t.run;
	t.drain_ntiles = (tiles + t.drain_run - 1u) / t.drain_run;
	/* (fewer post-stage tasks than workgroups set aside for them: the rest stay post workgroups -- consecutive blocks' tasks
	 * go round them -- and do NOT go to the DDC: its waves share the stream's frames evenly and wait for one another at the
	 * ring's end, so the launch runs at the pace of the fullest SIMD, r05) */
	return t;
}

/* ---- the streaming launch ---- */

/* LDS per workgroup: the post stage's stage and tile, or the DDC's NCO tables and window copies -- `nset` per buffer, two
 * buffers per wave (the block-boundary role inside the post workgroups lays its windows out the same way).  EVERY
 * workgroup of the launch reserves it (LDS is per kernel, not per role), so an audio filter of `nseg` x 64 taps decides how
 * many workgroups a CU's 160 KB hold: at D2 = 5, 40 064 / 56 448 / 89 216 B for 64 / 128 / 256 taps */
static inline size_t stream_lds_bytes(unsigned int d2, unsigned int nset, unsigned int nseg)
{
	const size_t post_lds = post_lds_bytes(d2, nseg) + 16u * sizeof(float);     /* (+ stream_post's `sh` words) */
	const size_t ddc_lds = (size_t)DDC_ROTATE_WAVES * 2u * 512u * nset + 2u * WR_SPLIT_N * 8u;
	return post_lds > ddc_lds ? post_lds : ddc_lds;
}

/* Which k_tuner_stream<PD2, NG, TS> a launch takes.  ONE channel filter for the whole tuner and an even number of lane
 * groups: NG = 2 (two lane groups share a wave's window and its reads).  Otherwise one lane group per wave: TS = 1 while
 * every lane group has a single channel filter (its own: hlane comes from the wave's lane group), TS = WR_TAPSETS
 * when a lane group mixes several.  (Two lane groups with different filters do not share a wave: NG = 2 stays the
 * one-filter shape, the one the headline runs, instruction for instruction.) */
static inline void stream_shape(unsigned int groups, unsigned int kmax, bool one_filter, unsigned int *ng, unsigned int *ts)
{
	*ng = (one_filter && !(groups & 1u)) ? 2u : 1u;
	*ts = kmax > 1u ? WR_TAPSETS : 1u;
}

static inline bool stream_nseg_supported(unsigned int d2, unsigned int nseg)
{
	return nseg == 1u || nseg == 2u || (nseg == 4u && d2 <= STREAM_NSEG4_MAX_D2);
}

/* the instance and the LDS request of a streaming launch; `ok` false: this launch shape cannot stream.  `kmax`: the most
 * channel filters a lane group of the launch mixes; `one_filter`: one for the whole tuner; `nseg`: the audio filter's taps / 64 */
struct WrStreamPlan {
	bool ok;
	unsigned int ng, ts;
	size_t lds;
};

static inline WrStreamPlan wrp_stream_plan(unsigned int d2, unsigned int groups, unsigned int kmax, bool one_filter,
                                           unsigned int nseg)
{
	WrStreamPlan p = {false, 0, 0, 0};
	if (!wrp_post_d2_supported(d2) || !stream_nseg_supported(d2, nseg) || !groups || groups > 16u || !kmax || kmax > WR_TAPSETS)
		return p;
	p.ok = true;
	stream_shape(groups, kmax, one_filter, &p.ng, &p.ts);
	p.lds = stream_lds_bytes(d2, p.ts == 1u ? 1u : kmax, nseg);
	return p;
}

/* How many workgroups of the streaming launch a device holds at once, split into roles.  Every workgroup of the
 * launch must be resident (they wait for one another): the grid is never larger than what the occupancy query (`per_cu`)
 * admits, capped at three per CU (what 80 registers and eight waves per workgroup give; the query can be one too
 * generous near a register-file edge, MI355X_MICROARCH.md "Residency").
 * An audio filter of 128 taps (and one of 256 up to D2 = 3) leaves a CU's LDS room for TWO workgroups, not three: one DDC
 * workgroup per CU instead of two, the post stage's slot as before.  Fewer than two: no launch (256 taps from D2 = 4 on),
 * and none on a device of four CUs or fewer, which has no post workgroup to give. */
struct WrStreamRoles {
	unsigned int n_ddc, n_post;            /* both 0: no launch */
};

static inline WrStreamRoles wrp_stream_roles(int per_cu, int num_cus)
{
	WrStreamRoles r = {0, 0};
	if (per_cu > 3)
		per_cu = 3;
	if (per_cu < 2 || num_cus <= 4)
		return r;
	/* the same number of DDC workgroups on every CU (see wrk_tuner_stream), one slot per CU for the post stage and the bell */
	r.n_ddc = (unsigned int)(per_cu - 1) * (unsigned int)num_cus;
	r.n_post = (unsigned int)num_cus - 4u;                  /* (three workgroup slots of the chip stay free: a copy kernel of the runtime's
	                                                           finds room without taking a slot the launch's own workgroups wait for) */
	return r;
}

/* ---- the per-block DDC, k_tuner_ddc<NCO, UTAPS, PD2, NG>.  Waves per workgroup, persistent workgroups per CU:
 *   ROTATE, uniform taps : 8 x 4 -- 64 VGPRs, 20 KiB of LDS: 8 waves per SIMD hide the recurrence's
 *                                  dependent FMAs better than 4 (measured 35.6 -> 34.7 us); NG = 2: 8 x 3
 *   ROTATE, per-lane taps: 8 x 4 -- one lane group's taps (16 KiB) per workgroup
 *   SPLIT                : 16 x 1 -- the replicated tables take 128 KiB
 *   EXACT                : 16 x 2 -- small LDS footprint, two workgroups hide the gather latency ---- */
struct WrDdcPlan {
	WrGroupMap map;                        /* ngroups 0: nothing to launch; rest: groups for further launches of their own */
	unsigned int ng;                       /* lane groups per wave: 2 where the launch allows (see k_tuner_ddc: NG), else 1 */
	unsigned int waves;                    /* per workgroup (W) */
	unsigned int kmax;
	size_t lds;
	unsigned int wgs_per_cu;               /* persistent DDC workgroups per CU, after the post reserve and the LDS fit */
	unsigned int post_wgs;                 /* workgroups of the riding post stage */
	unsigned int kslow, n_bnd;             /* block-boundary frames, and the workgroups that take them */
	size_t units;                          /* per wave and pass of its loop: NG lane groups */
	unsigned int wgs;                      /* the persistent ones; the grid is wgs + n_bnd + post_wgs */
};

/* `pd2`: the audio decimation of the riding post stage of `post_ntiles + 1` workgroups for each of `post_groups` lane groups,
 * or 0: none rides; `min_passes`: WR_TUNE_DDC_NG2_MIN_PASSES (0 = NG = 2 wherever the launch allows) */
static inline WrDdcPlan wrp_ddc_plan(int nco, bool utaps, unsigned int pd2, unsigned int slots_used, unsigned long long gsel,
                                     const unsigned char *nsets, bool one_filter, size_t k1, unsigned int d1, int num_cus,
                                     size_t min_passes, unsigned int post_ntiles, unsigned int post_groups)
{
	WrDdcPlan p;
	const bool rotate = nco == WR_NCO_ROTATE;
	const unsigned int W = p.waves = rotate ? DDC_ROTATE_WAVES : DDC_WAVES;
	p.map = wrp_group_map(slots_used, gsel);
	const unsigned int ngroups = p.map.ngroups;
	/* two lane groups per wave where the launch allows: an even number of lane groups, at most 16, all on one and the
	 * same channel filter ... and enough output frames: a wave of the NG = 2 kernel does twice the work per pass of its
	 * loop, so with few passes per wave the grid ends ragged (BASELINE config 5: 5 065 frames per chunk, 2.5 passes per
	 * wave -- 48 us against 43 with one lane group per wave); from four passes on the shared reads win */
	p.ng = 1u;
	if (rotate && utaps) {
		const size_t waves2 = (size_t)num_cus * (DDC_NG2_WAVES_PER_EU * 4u / W - (pd2 ? 1u : 0u)) * W;
		if (one_filter && !p.map.rest && ngroups >= 2u && (ngroups & 1u) == 0u && k1 * (ngroups / 2u) >= min_passes * waves2)
			p.ng = 2u;
	}
	/* tap sets: SPLIT one, its replicated tables leave no room for more windows */
	p.kmax = (utaps && rotate) ? wrp_kmax(p.map, nsets) : 1u;
	p.lds = (nco == WR_NCO_SPLIT) ? DDC_LDS_BYTES
	        : (W * 2u * 512u * p.kmax) + (rotate ? 2u * WR_SPLIT_N * 8u : 0u) + (rotate && !utaps ? WR_FIR_LENGTH * 64u * 4u : 0u);
	/* NG = 2: 80 registers, 6 waves per SIMD: three 8-wave workgroups per CU */
	p.wgs_per_cu = (p.ng == 2u) ? DDC_NG2_WAVES_PER_EU * 4u / W : rotate ? DDC_ROTATE_WGS_PER_CU : (nco == WR_NCO_EXACT) ? 2u : 1u;
	p.post_wgs = 0;
	if (pd2 != 0u) {
		/* the post workgroups' stage + tile set the LDS size of every workgroup of the launch;
		 * POST_RESERVE workgroup slots per CU are left to them (they come and go, the DDC ones
		 * persist).  Measured at C2, kernel duration (r02: per-slot turns, priorities by progress,
		 * post workgroups at priority 3): 1 slot 38.2 us, 2 slots 39.7, 3 slots 49.8 (the DDC
		 * starves); DDC + post as two launches: 31.3 + 15.2 + gap. */
		const size_t post_lds = post_lds_bytes(pd2, 1u);
		if (post_lds > p.lds)
			p.lds = post_lds;
		const unsigned int fit = (unsigned int)(WR_CU_LDS_BYTES / p.lds);
		if (fit < p.wgs_per_cu)
			p.wgs_per_cu = fit;
		const unsigned int POST_RESERVE = 1u;
		p.wgs_per_cu = (p.wgs_per_cu > POST_RESERVE) ? p.wgs_per_cu - POST_RESERVE : 1u;
		p.post_wgs = (post_ntiles + 1u) * post_groups;
	}
	/* launched even for a block too short to yield a channel-rate frame: workgroup 0 still
	 * advances the NCO (downconverter.cxx:103 runs per input frame) and rolls the histories */
	/* (roles: ROTATE with folded taps) the first ceil(63 / D1) output frames of the block reach into the previous one: they go
	 * to n_bnd workgroups of their own, one wave per (lane group, frame), and the persistent waves share the rest */
	p.kslow = (rotate && utaps) ? wrp_kslow(d1, k1) : 0u;
	p.n_bnd = (p.kslow * ngroups + W - 1u) / W;
	p.units = (k1 - p.kslow) * (ngroups / p.ng);
	p.wgs = (unsigned int)((p.units + W - 1) / W);
	const unsigned int cap = (unsigned int)num_cus * p.wgs_per_cu;
	if (p.wgs > cap)
		p.wgs = cap;                                        /* every slot: the kernel evens the units out (DDC_DEAL_WAYS) */
	if (rotate && !utaps) {
		/* per-lane taps live in LDS, one lane group per WORKGROUP: a whole number of
		 * workgroups per group, at least one */
		if (ngroups)
			p.wgs = (p.wgs / ngroups) * ngroups;
		if (p.wgs < ngroups)
			p.wgs = ngroups;
	} else {
		/* every lane group needs at least one wave of its own (the kernel deals waves to groups) */
		const unsigned int min_wgs = (ngroups / p.ng + W - 1) / W;
		if (p.wgs < min_wgs)
			p.wgs = min_wgs;
	}
	return p;
}

/* ---- the long-filter DDC (wrk_tuner_ddc_long).  `rot`: k_tuner_ddc_long_rot takes every frame and rolls the state
 * (a tolerance nco mode, one filter per lane group, a block with output frames); else k_tuner_ddc_long and
 * k_ddc_long_roll ---- */
struct WrLongPlan {
	bool rot;
	bool two;                              /* rot: two lane groups per wave (NG = 2) */
	unsigned int wgs_r, post_wgs, roll_wgs;/* rot: workgroups per role; the grid is their sum */
	size_t lds;                            /* rot */
	unsigned int wgs;                      /* the exact kernel's, 0: not launched */
	unsigned int rwgs;                     /* the roll kernel's */
};

/* `ride_d2`: the audio decimation of the riding post stage (as wrp_ddc_plan), or 0 */
static inline WrLongPlan wrp_long_plan(bool rotate, bool one_filter, size_t k1, unsigned int groups, unsigned int len,
                                       unsigned int slots, int num_cus, unsigned int ride_d2, unsigned int post_ntiles,
                                       unsigned int post_groups)
{
	WrLongPlan p = {false, false, 0, 0, 0, 0, 0, 0};
	const size_t roll_total = (size_t)(len - 1u) * slots;
	p.rot = rotate && k1;
	if (p.rot) {
		const size_t units_r = k1 * groups;
		p.two = one_filter && groups % 2u == 0;
		p.wgs_r = (unsigned int)(((p.two ? units_r / 2 : units_r) + LONG_ROT_WAVES - 1u) / LONG_ROT_WAVES);
		/* persistent: 32 waves per CU as before -- or 24 and one workgroup slot per CU left to the post workgroups, which
		 * come and go beside the DDC ones (as in k_tuner_ddc) instead of queueing up behind them */
		const unsigned int cap8 = (unsigned int)num_cus * (ride_d2 ? 3u : 4u);
		if (p.wgs_r > cap8)
			p.wgs_r = cap8;
		p.post_wgs = ride_d2 ? (post_ntiles + 1u) * post_groups : 0u;
		const size_t roll_wgs = (roll_total + LONG_ROT_WAVES * 64u - 1u) / (LONG_ROT_WAVES * 64u);
		p.roll_wgs = roll_wgs > 256u ? 256u : (unsigned int)roll_wgs;
		p.lds = LONG_ROT_LDS;
		if (ride_d2 && post_lds_bytes(ride_d2, 1u) > p.lds)
			p.lds = post_lds_bytes(ride_d2, 1u);
		return p;
	}
	const size_t units = k1 * groups;
	p.wgs = (unsigned int)((units + 3) / 4);
	const unsigned int cap = (unsigned int)num_cus * 8u;
	if (p.wgs > cap)
		p.wgs = cap;
	p.rwgs = (unsigned int)((roll_total + 255) / 256 > 1024 ? 1024 : (roll_total + 255) / 256);
	return p;
}

/* ---- the audio filter on its own (wrk_tuner_audio): `len` taps, 64 or 128 / 256 ---- */
struct WrAudioPlan {
	unsigned int tk;                       /* output frames per tile: as many as the staged rows allow */
	unsigned int need;                     /* staged rows */
	size_t lds;                            /* sized to what this decimation needs, so that two workgroups fit a CU when D2 is small */
	size_t lds_max;                        /* the most the kernel asks for: 156 KiB of 160 */
	unsigned int grid_x;                   /* tiles; grid.y is the lane groups */
};

static inline WrAudioPlan wrp_audio_plan(size_t k2, unsigned int d2, unsigned int len)
{
	WrAudioPlan p;
	p.tk = AUD_TMAX;
	if (d2 > 1 && (AUD_ROWS - len) / d2 + 1u < p.tk)
		p.tk = (AUD_ROWS - len) / d2 + 1u;
	p.need = (p.tk - 1u) * d2 + len;
	p.lds = ((size_t)p.need * 64u + (size_t)len * 64u + AUD_TMAX * 65u) * sizeof(float);
	p.lds_max = ((size_t)AUD_ROWS * 64u + (size_t)WR_FIR_FUSED_MAX * 64u + AUD_TMAX * 65u) * sizeof(float);
	p.grid_x = (unsigned int)((k2 + p.tk - 1) / p.tk);
	return p;
}

/* ---- the spectrum launches (wr_fft.hip): a transform of `points` complex points -- the frame's n, or n / 2 packed points of
 * a real frame (channels == 1) -- lives in two LDS buffers of at most FFT_LDS_POINTS points each ---- */
#define FFT_THREADS 256
#define FFT_LDS_POINTS 8192u               /* per buffer: 64 KiB of float2 */
#define FFT_LDS_MAX ((size_t)2 * FFT_LDS_POINTS * 8u)   /* the most dynamic LDS an FFT kernel asks for: 128 KiB */
#define FFT_TILE_MAX 16u                   /* columns (pass 1) or rows (pass 2) of a four-step workgroup */
#define FFT_COLS_CT_MAX 8u                 /* columns per workgroup of k_fft_cols: 64-byte runs */
#define FFT_WORK_BYTES ((size_t)128 << 20) /* the work area between the passes: it then still sits in the 256 MB Infinity Cache */
#define SPEC_AVG_BYTES ((size_t)64 << 20)  /* wr_spectrum_batch_avg's scratch (bins and carry): the 127 frames of a BASELINE config 3
                                              block in one chunk, and with the work area above still inside the Infinity Cache */
#define SPEC_REDUCE_THREADS 256u           /* k_spec_reduce: one thread per (group, bin) */
#define SPEC_ROWS_GRID_CAP 4096u           /* k_rows_waterfall strides beyond 2^20 (row, column) pairs */
#define FFT_DB_GRID_CAP 1024u              /* k_bins_to_db strides beyond 262144 bins */
#define FFT_WATERFALL_GRID_CAP 4096u       /* k_waterfall_row: 2^20 columns, the largest transform's; never reached below it */
/* batches of the 65536-point path from this many frames on take four frames per pass-1 workgroup (>= 384 workgroups) */
#define FFT64K_P1_LONG_MIN 96u

enum WrFftPath {
	WR_FFT_SINGLE = 0,                     /* one workgroup per frame, whole in LDS */
	WR_FFT_FOUR_STEP,                      /* points = n1 * n2, two launches with the work area between them */
	WR_FFT_REG64K                          /* 65536 IQ points: 256 x 256 with the sub-transforms in registers */
};

struct WrFftShape {
	unsigned int points, n1, n2;           /* n2 == 1: single-pass */
	unsigned int sub;                      /* length of the sub-transforms' twiddle table, max(n1, n2); 0: single-pass */
	WrFftPath path;
	size_t lds_max;
	bool real;                             /* the packed transform of a real frame: an untangle step follows */
};

/* up to FFT_LDS_POINTS points a single pass; above, n1 = 2^ceil(bits / 2) */
static inline WrFftShape wrp_fft_shape(unsigned int n, unsigned int channels)
{
	WrFftShape s = {channels == 1u ? n / 2u : n, 0, 1, 0, WR_FFT_SINGLE, FFT_LDS_MAX, channels == 1u};
	s.n1 = s.points;
	if (s.points > FFT_LDS_POINTS) {
		unsigned int bits = 0;
		while ((1u << bits) < s.points)
			bits++;
		s.n1 = 1u << ((bits + 1u) / 2u);
		s.n2 = s.points / s.n1;
		s.sub = s.n1 > s.n2 ? s.n1 : s.n2;
		s.path = (!s.real && s.points == 65536u) ? WR_FFT_REG64K : WR_FFT_FOUR_STEP;
	}
	return s;
}

/* one batch of `batch` frames.  Single-pass: lds1, grid (g1x).  Four-step: ct columns / rt rows per workgroup, as many as
 * the LDS holds and FFT_TILE_MAX at most, grids (n2 / ct, batch) and (n1 / rt, batch) and, real plans, the untangle step's
 * (m / FFT_THREADS, batch).  Register path: static LDS, fpw frames per pass-1 workgroup, (16, ceil(batch / fpw)) and (16, batch). */
struct WrFftLaunch {
	unsigned int ct, rt, fpw;
	size_t lds1, lds2;
	unsigned int g1x, g1y, g2x, g2y, g3x, g3y;     /* 0: no such launch */
};

static inline WrFftLaunch wrp_fft_launch(const WrFftShape &s, size_t batch)
{
	WrFftLaunch l = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	const unsigned int b = (unsigned int)batch;
	if (s.path == WR_FFT_SINGLE) {
		l.lds1 = (size_t)2 * s.points * 8u;
		l.g1x = b;
		l.g1y = 1;
	} else if (s.path == WR_FFT_REG64K) {
		l.fpw = batch >= FFT64K_P1_LONG_MIN ? 4u : 1u;
		l.g1x = l.g2x = 16;
		l.g1y = (b + l.fpw - 1u) / l.fpw;
		l.g2y = b;
	} else {
		l.ct = FFT_LDS_POINTS / s.n1 > FFT_TILE_MAX ? FFT_TILE_MAX : FFT_LDS_POINTS / s.n1;
		l.rt = FFT_LDS_POINTS / s.n2 > FFT_TILE_MAX ? FFT_TILE_MAX : FFT_LDS_POINTS / s.n2;
		l.lds1 = (size_t)2 * s.n1 * l.ct * 8u;
		l.lds2 = (size_t)2 * s.n2 * l.rt * 8u;
		l.g1x = s.n2 / l.ct;
		l.g2x = s.n1 / l.rt;
		l.g1y = l.g2y = b;
		if (s.real) {
			l.g3x = s.points / FFT_THREADS;
			l.g3y = b;
		}
	}
	return l;
}

/* The work area of a two-pass plan of n-point frames (8 n bytes each: a real plan's two halves are n / 2 points): room for
 * the whole batch, up to FFT_WORK_BYTES, means one pair of launches per call instead of one per 64 frames.  Grows only:
 * the frames it holds after a call for `want_frames`, `have` before. */
static inline size_t wrp_fft_work_frames(unsigned int n, size_t have, size_t want_frames)
{
	size_t want = FFT_WORK_BYTES / ((size_t)n * 8u);
	if (want < 1)
		want = 1;
	if (want > want_frames)
		want = want_frames;
	return want > have ? want : have;
}

/* a call's frames go through the work area in chunks */
static inline size_t wrp_fft_chunk(size_t remaining, size_t work_frames)
{
	return remaining < work_frames ? remaining : work_frames;
}

/* a real plan (m = n / 2 packed points): of the work area's work_frames * n complex values the first half is the intermediate
 * between the passes, the second -- from this offset on -- the packed transform Z that the untangle step reads */
static inline size_t wrp_fft_untangle_offset(size_t work_frames, unsigned int m)
{
	return work_frames * m;
}

/* columns per workgroup of k_fft_cols.  Workgroups first: measured at 256 columns (profiles/chan_spectra.txt), one column
 * per workgroup -- 256 workgroups, 8-byte loads a row apart -- takes 5.2 us at n = 512 where 8 columns in 32 workgroups, 64-byte
 * runs per row, take 17.4.  So columns are put side by side only where there are more of them than compute units, and
 * then within what the LDS holds: both buffers within 128 KiB (n * ct <= 8192 points, k_fft_single's budget at 8192), at
 * most 8 (64-byte runs).  A power of two: it divides 64.  (num_cus <= 0: the rule without the compute units.) */
static inline unsigned int wrp_fft_cols_ct(unsigned int n, unsigned int cols, int num_cus)
{
	unsigned int most = FFT_LDS_POINTS / n;
	if (most > FFT_COLS_CT_MAX)
		most = FFT_COLS_CT_MAX;
	if (num_cus > 0 && most > cols / (unsigned int)num_cus)
		most = cols / (unsigned int)num_cus;
	unsigned int ct = 1;
	while (2u * ct <= most)
		ct *= 2u;
	return ct;
}

/* ---- wr_spectrum_batch_avg: `G` groups of `F` frames of n points each.  The transforms write bins into a scratch area of
 * at most SPEC_AVG_BYTES (8 n bytes a frame: 8 frames of 2^20 points, 2^20 frames of 8), k_spec_reduce walks them.  A chunk
 * is `ng` whole groups of `nf` frames each:
 *   F frames fit the area : every chunk takes all F frames of as many groups as fit, gchunk at most
 *   they do not           : one group at a time, fchunk frames per chunk, and one frame's worth of the area is the carry
 *                           buffer that hands sum and peak from a chunk to the next (carry = 1 group)
 * Groups are the outer loop, a group's frames go in order. ---- */
struct WrSpecAvgPlan {
	size_t fchunk, gchunk;                 /* frames of a group and groups per chunk, at most */
	size_t carry;                          /* groups the carry buffer holds: 0 where no group's frames are cut */
};

static inline WrSpecAvgPlan wrp_spec_avg_plan(unsigned int n, size_t F, size_t G)
{
	WrSpecAvgPlan p = {0, 0, 0};
	const size_t room = SPEC_AVG_BYTES / ((size_t)n * 8u);      /* frames; 8 or more */
	if (!F || !G)
		return p;
	if (F <= room) {
		p.fchunk = F;
		p.gchunk = room / F < G ? room / F : G;
	} else {
		p.fchunk = room - 1u;
		p.gchunk = 1;
		p.carry = 1;
	}
	return p;
}

/* the scratch area of a plan: bins [gchunk][fchunk][n][2], then the carry [carry][n][2] (sum, peak) */
static inline size_t wrp_spec_avg_bytes(unsigned int n, const WrSpecAvgPlan &p)
{
	return (p.fchunk * p.gchunk + p.carry) * (size_t)n * 8u;
}

struct WrSpecAvgChunk {
	size_t g0, ng, f0, nf;                 /* groups [g0, g0 + ng), of each frames [f0, f0 + nf) */
};

/* the chunk behind `c` (`start`: the first); false: there is none */
static inline bool wrp_spec_avg_next(const WrSpecAvgPlan &p, size_t F, size_t G, WrSpecAvgChunk *c, bool start)
{
	if (!p.fchunk || !p.gchunk)
		return false;
	if (start) {
		c->g0 = 0;
		c->f0 = 0;
	} else if (c->f0 + c->nf < F) {
		c->f0 += c->nf;
	} else {
		c->g0 += c->ng;
		c->f0 = 0;
	}
	if (c->g0 >= G)
		return false;
	c->ng = G - c->g0 < p.gchunk ? G - c->g0 : p.gchunk;
	c->nf = F - c->f0 < p.fchunk ? F - c->f0 : p.fchunk;
	return true;
}

/* k_spec_reduce on a chunk of `ng` groups: a thread per (group, bin), no stride (ng * n <= SPEC_AVG_BYTES / 8) */
static inline unsigned int wrp_spec_reduce_grid(unsigned int n, size_t ng)
{
	return (unsigned int)((ng * n + SPEC_REDUCE_THREADS - 1u) / SPEC_REDUCE_THREADS);
}

/* launches of one chunk.  Single-workgroup sizes: the transform of all its groups' frames and the reduce, however many
 * groups.  Two-pass sizes: the transform is a loop over the groups, each through the work area (`work_frames` frames) in
 * pieces of two launches (real: three), and the reduce. */
static inline size_t wrp_spec_avg_chunk_launches(const WrFftShape &s, size_t ng, size_t nf, size_t work_frames)
{
	if (s.path == WR_FFT_SINGLE)
		return 2;
	const size_t pieces = (nf + work_frames - 1u) / work_frames;
	return ng * pieces * (s.real ? 3u : 2u) + 1u;
}

/* launches of a whole call (closed form of the loop over wrp_spec_avg_next) */
static inline size_t wrp_spec_avg_launches(unsigned int n, unsigned int channels, size_t F, size_t G, size_t work_frames)
{
	const WrFftShape s = wrp_fft_shape(n, channels);
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	if (!p.fchunk)
		return 0;
	const size_t gfull = G / p.gchunk, grem = G % p.gchunk, ffull = F / p.fchunk, frem = F % p.fchunk;
	size_t total = gfull * ffull * wrp_spec_avg_chunk_launches(s, p.gchunk, p.fchunk, work_frames);
	if (frem)
		total += gfull * wrp_spec_avg_chunk_launches(s, p.gchunk, frem, work_frames);
	if (grem) {
		total += ffull * wrp_spec_avg_chunk_launches(s, grem, p.fchunk, work_frames);
		if (frem)
			total += wrp_spec_avg_chunk_launches(s, grem, frem, work_frames);
	}
	return total;
}

/* k_rows_waterfall: a thread per (row, pixel column) */
static inline unsigned int wrp_rows_waterfall_grid(size_t nrows, unsigned int width)
{
	return grid_for(nrows * width, 256, SPEC_ROWS_GRID_CAP);
}

/* ---- wr_spectrum_rows_detect: two launches per chunk of rows.  k_detect_floor: a workgroup per (row, span), its histogram
 * and digit hand-off in LDS and, where the span fits, the span's keys behind them.  k_detect_segments: a workgroup per row,
 * tiles of DETECT_TILE bins, DETECT_PER consecutive bins a thread.  Floors of a chunk: [rows][nspans] floats, within
 * DETECT_FLOOR_BYTES -- which one row of 2^20 points in spans of 8 fills. ---- */
#define DETECT_THREADS     256u
#define DETECT_PER         4u
#define DETECT_TILE        (DETECT_THREADS * DETECT_PER)
#define DETECT_WAVES       (DETECT_THREADS / 64u)
#define DETECT_LDS_KEYS    8192u                   /* a span of up to this many bins keeps its keys in LDS (32 KiB) */
#define DETECT_FLOOR_HEAD  (256u + 4u)             /* dwords in front of the keys: the histogram, the chosen digit's hand-off */
#define DETECT_SEG_LDS     (DETECT_WAVES * (2u * 4u + 4u + 24u + 4u))   /* k_detect_segments: the waves' hot flags (two sets), the wave totals of its three scans */
#define DETECT_FLOOR_BYTES ((size_t)512 << 10)
#define DETECT_WG_LDS_MAX  (64u * 1024u)           /* what a workgroup may have without asking */

/* the field of the rule that breaks a limit on rows of n floats, or NULL */
static inline const char *wrp_detect_rule_bad(unsigned int n, const wr_detect_rule *r)
{
	if (r->bin0 > n || r->nbins > n - r->bin0)
		return "bin0";
	if (r->nbins < 8u)
		return "nbins";
	if (r->span < 8u || r->span > r->nbins || r->nbins % r->span)
		return "span";
	if (r->percent > 100u)
		return "percent";
	if (!(r->threshold - r->threshold == 0.0f))             /* NaN, +-inf */
		return "threshold";
	if (r->max_gap > r->nbins)
		return "max_gap";
	if (r->min_width < 1u || r->min_width > r->nbins)
		return "min_width";
	return NULL;
}

struct WrDetectPlan {
	unsigned int nspans;                   /* floors of a row */
	size_t chunk_rows;                     /* rows of a chunk, at most */
	size_t floor_bytes;                    /* the floors of the call's largest chunk */
	bool keys_in_lds;
	size_t lds_floor, lds_segments;        /* bytes */
};

/* a valid rule (wrp_detect_rule_bad) */
static inline WrDetectPlan wrp_detect_plan(const wr_detect_rule *r, size_t nrows)
{
	WrDetectPlan p;
	p.nspans = r->nbins / r->span;
	p.chunk_rows = DETECT_FLOOR_BYTES / 4u / p.nspans;              /* 1 or more: nspans <= 2^20 / 8 */
	p.floor_bytes = (nrows < p.chunk_rows ? nrows : p.chunk_rows) * p.nspans * 4u;
	p.keys_in_lds = r->span <= DETECT_LDS_KEYS;
	p.lds_floor = (DETECT_FLOOR_HEAD + (p.keys_in_lds ? r->span : 0u)) * 4u;
	p.lds_segments = DETECT_SEG_LDS;
	return p;
}

/* the chunk behind rows [*r0, *r0 + *nr) (`start`: the first); false: there is none */
static inline bool wrp_detect_next(const WrDetectPlan &p, size_t nrows, size_t *r0, size_t *nr, bool start)
{
	*r0 = start ? 0 : *r0 + *nr;
	if (*r0 >= nrows)
		return false;
	*nr = nrows - *r0 < p.chunk_rows ? nrows - *r0 : p.chunk_rows;
	return true;
}

/* a chunk's grids: k_detect_floor, a workgroup per (row, span) -- 2^17 at most; k_detect_segments, a workgroup per row */
static inline unsigned int wrp_detect_floor_grid(const WrDetectPlan &p, size_t rows)
{
	return (unsigned int)(rows * p.nspans);
}

static inline unsigned int wrp_detect_segments_grid(size_t rows)
{
	return (unsigned int)rows;
}

/* ---- the voice bank (wr_voice.hip, k_voice_rows): a workgroup is one wave and VOICE_CHUNK consecutive outputs of one row,
 * VOICE_PER consecutive outputs a thread; its input span of VOICE_CHUNK + T - 1 frames lies in LDS behind four floats that
 * the last look-ahead read of thread 0 touches.  The grid is (chunks + 1) x rows: the extra workgroup of a row writes its new
 * history.  One wave per workgroup: a push of 256 rows of 2 000 frames is two thousand waves, two per SIMD of the chip, and
 * they spread best one at a time (wr_voice.hip: why four outputs a thread and not eight). ---- */
#define VOICE_THREADS    64u
#define VOICE_PER        4u
#define VOICE_CHUNK      256u               /* VOICE_THREADS * VOICE_PER */
#define VOICE_T_MIN      8u
#define VOICE_T_MAX      2048u
#define VOICE_FILTERS    16u
#define VOICE_LDS_FLOATS (4u + VOICE_CHUNK + VOICE_T_MAX)   /* 9 232 bytes */

/* the header's limits on a filter length */
static inline bool wrp_voice_len_ok(unsigned int T)
{
	return T >= VOICE_T_MIN && T <= VOICE_T_MAX && !(T & 3u);
}

struct WrVoicePlan {
	unsigned int chunks;                   /* workgroups of a row that compute outputs */
	unsigned int grid_x;                   /* ... and the one that writes the row's history; grid.y is the rows */
	unsigned int threads;
};

/* a push of `nframes` frames, 1 .. 2^28 */
static inline WrVoicePlan wrp_voice_plan(size_t nframes)
{
	WrVoicePlan p;
	p.chunks = (unsigned int)((nframes + VOICE_CHUNK - 1u) / VOICE_CHUNK);
	p.grid_x = p.chunks + 1u;
	p.threads = VOICE_THREADS;
	return p;
}

/* ================================================================== the row kernels ================================== */

/* ---- the tone bank (wr_tones.hip): k_tones_part, a workgroup of TN_WAVES waves per TN_CHUNK frames of a row, then
 * k_tones_latch, a workgroup of one wave per row ---- */
#define TN_THREADS 256u
#define TN_WAVES   (TN_THREADS / WR_LANES)
#define TN_RUN     128u                        /* frames a wave walks */
#define TN_CHUNK   (TN_RUN * TN_WAVES)         /* frames of a workgroup */
#define TN_TABLE   4096u
#define TN_WINDOW_MIN 16u
#define TN_WINDOW_MAX 65536u

struct WrTonesPlan {
	size_t chunks;                         /* grid.x of k_tones_part (grid.y: the rows); above 2^31 - 1: no launch */
	unsigned long long nq;                 /* the push is nq * window + nr frames */
	unsigned int nr;
};

static inline WrTonesPlan wrp_tones_plan(size_t nframes, unsigned int window)
{
	WrTonesPlan p;
	p.chunks = (nframes + TN_CHUNK - 1u) / TN_CHUNK;
	p.nq = nframes / window;
	p.nr = (unsigned int)(nframes % window);
	return p;
}

/* the two stretches of a push for a row with `fill` frames in its open window: A = [a_lo, b_lo) counted from frame `oa`
 * of the push (which may lie in front of it), B = [b_lo, nframes) counted from `ob`; the push is nq * W + nr frames */
struct WrTonesCut {
	long long a_lo, b_lo, oa, ob;
	unsigned long long ends;
	unsigned int fill_after;
};

WRP_HD WrTonesCut wrp_tones_cut(unsigned int fill, unsigned long long nq, unsigned int nr, unsigned int W)
{
	WrTonesCut c;
	const bool over = nr + fill >= W;              /* fill < W, nr < W */
	c.ends = nq + (over ? 1u : 0u);
	c.fill_after = nr + fill - (over ? W : 0u);
	if (!c.ends) {
		c.a_lo = c.b_lo = c.oa = 0;
		c.ob = -(long long)fill;
	} else {
		const long long e = (long long)(c.ends * W) - (long long)fill;
		c.oa = e - (long long)W;
		c.a_lo = c.oa > 0 ? c.oa : 0;
		c.b_lo = c.ob = e;
	}
	return c;
}

/* ---- the DCS bank (wr_dcs.hip): k_dcs_push, a workgroup per row.  The clock is frames * step in units of 2^-29 chip; a
 * launch takes frames whose chips, the next frame's included, lie within DC_SPAN of its first ---- */
#define WR_DCS_CODES 128                   /* code words a bank holds at most: a lane each, two waves */
#define WR_DCS_RING  512                   /* chip sums a row keeps, indexed by chip mod 512 (wr_dcs.hip: why that many) */
#define DC_THREADS 256u
#define DC_RING    WR_DCS_RING
#define DC_SPAN    256u                          /* chips a launch may touch, the chip of the frame behind it included */
#define DC_BACK    191u                          /* chips an evaluation reaches back from the first it does not use */
#define DC_CAND    (8u * 23u)
#define DC_CHIP_BITS 29u                         /* a chip is 2^29 units of the clock: an eighth of a bit of 2^32 */
#define DC_STEP_MIN (1u << 19)                   /* 1024 frames a chip */
#define DC_STEP_MAX (1u << 28)                   /* 2 frames a chip */

static_assert(DC_BACK + 1u + DC_SPAN <= DC_RING, "a launch's live chips must fit the ring");
static_assert((DC_RING & (DC_RING - 1u)) == 0, "the ring is indexed by g mod DC_RING");

static inline bool wrp_dcs_step_ok(unsigned long long step)
{
	return step >= DC_STEP_MIN && step <= DC_STEP_MAX;
}

/* where a launch begins: its first frame's chip and how far into the chip that frame lies */
struct WrDcsAt {
	unsigned long long g0;
	unsigned int ph0;                      /* < 2^29 */
};

/* the start of a push at clock `first_frame`: the product may pass 2^64 and is reduced here */
static inline WrDcsAt wrp_dcs_start(unsigned long long first_frame, unsigned int step)
{
	const unsigned __int128 at = (unsigned __int128)first_frame * step;
	const WrDcsAt a = {(unsigned long long)(at >> DC_CHIP_BITS), (unsigned int)((unsigned long long)at & ((1u << DC_CHIP_BITS) - 1u))};
	return a;
}

/* the most frames n a launch at `at` may take, (ph0 + n * step) >> 29 < DC_SPAN: 510 or more, step being 2^28 at most */
static inline size_t wrp_dcs_room(const WrDcsAt &at, unsigned int step)
{
	return (size_t)((((unsigned long long)DC_SPAN << DC_CHIP_BITS) - 1u - at.ph0) / step);
}

/* the frames the launch at `at` takes of the `left` a push still has ... */
static inline size_t wrp_dcs_take(const WrDcsAt &at, unsigned int step, size_t left)
{
	const size_t room = wrp_dcs_room(at, step);
	return left < room ? left : room;
}

/* ... and where the launch behind it begins */
static inline WrDcsAt wrp_dcs_after(const WrDcsAt &at, unsigned int step, size_t n)
{
	const unsigned long long a = at.ph0 + (unsigned long long)n * step;
	const WrDcsAt b = {at.g0 + (a >> DC_CHIP_BITS), (unsigned int)(a & ((1u << DC_CHIP_BITS) - 1u))};
	return b;
}

/* ---- the resampler (wr_resamp.hip): k_resamp_rows, a workgroup per RS_THREADS consecutive outputs of a row and one more
 * per row for its history.  The header's limits on (L, M, P) are what the chunk's input span in LDS rests on ---- */
#define RS_THREADS   256u
#define RS_L_MAX     1024u
#define RS_RATIO_MAX 8u                    /* M <= 8 L and L <= 8 M */
#define RS_P_MIN     4u
#define RS_P_MAX     64u                   /* and a multiple of 4 */
#define RS_TAPS_MAX  16384u                /* L * P: the table is at most 64 KiB */
#define RS_SPAN      2112u                 /* floats of LDS for a chunk's input span */

/* the worst span: rem0 = L - 1, cnt = RS_THREADS, M = 8 L, P = 64 -- (L - 1 + 255 * 8 L) / L + 64 = 2104 */
static_assert((RS_L_MAX - 1u + (RS_THREADS - 1u) * RS_RATIO_MAX * RS_L_MAX) / RS_L_MAX + RS_P_MAX == 2104u &&
              2104u <= RS_SPAN, "RS_SPAN covers the longest input span the limits allow");

/* non-zero: (L, M, P) break the header's limits */
static inline int wrp_resamp_limits_bad(unsigned int L, unsigned int M, unsigned int P)
{
	return !L || L > RS_L_MAX || !M || M > RS_RATIO_MAX * L || L > RS_RATIO_MAX * M || P < RS_P_MIN || P > RS_P_MAX || (P & 3u) ||
	       L * P > RS_TAPS_MAX;
}

/* the output frames a push of `nframes` yields at clock `nmod` = N mod M: ceil((nmod + nframes) L / M) - ceil(nmod L / M) */
static inline unsigned long long wrp_resamp_out_frames(unsigned int L, unsigned int M, unsigned int nmod, unsigned long long nframes)
{
	const unsigned long long a = ((unsigned long long)nmod * L + M - 1u) / M;
	const unsigned long long b = (((unsigned long long)nmod + nframes) * L + M - 1u) / M;
	return b - a;
}

struct WrResampPlan {
	unsigned long long n_out;              /* output frames of a row */
	unsigned int j0;                       /* ceil(nmod L / M): output i of the push is frame q L + j0 + i of the stream */
	unsigned int chunks;                   /* workgroups of a row that compute outputs; <= 2^23 */
	unsigned int grid_x;                   /* ... and the one that writes the row's history; grid.y is the rows */
};

/* a push of `nframes` frames, 1 .. 2^28, within the limits */
static inline WrResampPlan wrp_resamp_plan(unsigned int L, unsigned int M, unsigned int nmod, size_t nframes)
{
	WrResampPlan p;
	p.n_out = wrp_resamp_out_frames(L, M, nmod, nframes);
	p.j0 = (unsigned int)(((unsigned long long)nmod * L + M - 1u) / M);
	p.chunks = (unsigned int)((p.n_out + RS_THREADS - 1u) / RS_THREADS);
	p.grid_x = p.chunks + 1u;
	return p;
}

/* chunk `chunk` < chunks of a row: outputs [i0, i0 + cnt) of the push.  The first of them reads the push's frame `base`
 * (n0 - N0 >= 0) at phase rem0 < L; the chunk's inputs are `span` frames from frame lo = base - (P - 1) >= -(P - 1) on */
struct WrResampChunk {
	unsigned long long i0;
	long long base, lo;
	unsigned int rem0, cnt, span;
};

WRP_HD WrResampChunk wrp_resamp_chunk(unsigned int L, unsigned int M, unsigned int P, unsigned int nmod, unsigned int j0,
                                      unsigned long long n_out, unsigned int chunk)
{
	WrResampChunk c;
	c.i0 = (unsigned long long)chunk * RS_THREADS;
	const unsigned long long u0 = ((unsigned long long)j0 + c.i0) * M;
	c.base = (long long)(u0 / L) - (long long)nmod;
	c.rem0 = (unsigned int)(u0 % L);
	const unsigned long long left = n_out - c.i0;
	c.cnt = left < RS_THREADS ? (unsigned int)left : RS_THREADS;
	c.lo = c.base - (long long)(P - 1u);
	c.span = (c.rem0 + (c.cnt - 1u) * M) / L + P;
	return c;
}

/* ---- signal levels (wr_levels.hip): k_levels_part, a workgroup of LV_RUNS waves per group of LV_ROWS rows and lane group of
 * columns, then k_levels_sum, a thread per column over the groups.  The work area, in floats: the groups' sums, peaks and
 * muted counts, [groups][cols] each, then the result [3][cols] ---- */
#define LV_RUN     16u                     /* frames of a run = rows a lane has in flight */
#define LV_RUNS    16u                     /* runs of a group = waves of a workgroup */
#define LV_ROWS    (LV_RUN * LV_RUNS)      /* rows of a group */
#define LV_THREADS (LV_RUNS * WR_LANES)
#define LV_SUM_THREADS 256u

struct WrLevelsPlan {
	size_t groups;                         /* grid.x of k_levels_part; above 2^31 - 1: no launch */
	unsigned int grid_y;                   /* lane groups of columns */
	size_t lds_squelch;                    /* dynamic LDS of the instance that counts muted frames: a group's e values, 64 KiB */
	unsigned int sum_grid;                 /* k_levels_sum */
	size_t psum, ppeak, pmuted, res;       /* offsets into the work area, floats */
	size_t work_floats;                    /* ... and its size */
};

static inline WrLevelsPlan wrp_levels_plan(unsigned int cols, size_t k1)
{
	WrLevelsPlan p;
	p.groups = (k1 + LV_ROWS - 1u) / LV_ROWS;
	p.grid_y = (cols + WR_LANES - 1u) / WR_LANES;
	p.lds_squelch = (size_t)LV_ROWS * WR_LANES * sizeof(float);
	p.sum_grid = (cols + LV_SUM_THREADS - 1u) / LV_SUM_THREADS;
	p.psum = 0;
	p.ppeak = p.groups * cols;
	p.pmuted = 2u * p.groups * cols;
	p.res = 3u * p.groups * cols;
	p.work_floats = (p.groups + 1u) * 3u * cols;
	return p;
}

/* ---- audio AGC (wr_agc.hip): k_agc_rows, a workgroup per row (the grid is the rows) walks it in tiles of AGC_TILE frames,
 * AGC_PER a thread ---- */
#define AGC_THREADS 256u
#define AGC_PER     4u                          /* consecutive frames of a thread */
#define AGC_TILE    (AGC_THREADS * AGC_PER)
#define AGC_WAVES   (AGC_THREADS / WR_LANES)

#endif /* WR_PLAN_H_ */
