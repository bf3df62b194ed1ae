/*
 * wr_tuner_submit.hip -- a tuner's upload and submit path: what a rate group's filters amount to and their upload
 * (wrc_group_upload), the profiling event pairs, a block's way through the launch sequence (wrc_tuner_submit_now), the
 * blocks held for one launch, and the launch marks.  The tuner itself is in wr_tuner.hip, what reads a submit's results
 * back in wr_tuner_read.hip.
 */
#include "wr_capi_internal.h"

/* what the host shadow of a group's filters amounts to, lane group by lane group: group_classify looks (and notes
 * what it finds in the Group's own flags, masks and counts), wrc_group_upload copies */
namespace {                              /* (its destructor is no name of the library's) */
struct GroupFilters {
	std::vector<float> taps1u;           /* [lane groups][WR_TAPSETS][64], window order */
	std::vector<float> taps2u;           /* [lane groups][l2] */
	std::vector<int> tapsel;             /* slot -> its set in taps1u */
};
}

/* the representative of the lane group at `base` -- its first channel, -1: it has none -- and whether every channel
 * of the lane group has the representative's `len` taps at taps(channel) */
template <typename Taps>
static int lane_group_rep(const wr_tuner *t, const Group *g, size_t base, Taps taps, unsigned int len, bool *same)
{
	int rep = -1;
	*same = true;
	for (size_t s = base; s < base + WR_LANES && *same; ++s) {
		const int ci = g->owner[s];
		if (ci < 0)
			continue;
		if (rep < 0)
			rep = ci;
		else
			*same = !memcmp(taps(t->chans[ci]), taps(t->chans[rep]), sizeof(float) * len);
	}
	return rep;
}

static void group_classify(const wr_tuner *t, Group *g, GroupFilters &F)
{
	const size_t S = g->slots;
	/* Receivers of a tuner nearly always share one channel filter (radio.cxx:78-79 sets the same
	 * passband/rate for all), and when they do not (receiverhandler.cxx:130-137: every receiver has
	 * its own passband control) a lane group still holds only a few distinct ones.  The fast kernel
	 * folds the taps into the shared sample window, one copy of the window per distinct filter (up
	 * to WR_TAPSETS); a lane group with more than that takes the per-lane-taps kernel. */
	int first_rep = -1;                  /* a channel of the first lane group that has any */
	g->uniform_taps = g->one_filter = true;
	g->uniform_mask = g->fewsets_mask = g->uniform2_mask = 0;
	memset(g->nsets, 0, sizeof(g->nsets));
	F.taps1u.assign(S * WR_TAPSETS, 0.0f);
	F.tapsel.assign(S, 0);
	for (size_t base = 0; base < S; base += WR_LANES) {
		const size_t grp = base / WR_LANES;
		int reps[WR_TAPSETS];
		unsigned int nrep = 0;
		bool few = true;
		for (size_t s = base; s < base + WR_LANES; ++s) {
			int ci = g->owner[s];
			if (ci < 0)
				continue;
			unsigned int q = 0;
			for (; q < nrep; ++q)
				if (!memcmp(t->chans[ci].taps[0], t->chans[reps[q]].taps[0], sizeof(float) * WR_FIR_LENGTH))
					break;
			if (q == nrep) {
				if (nrep == WR_TAPSETS) {
					few = false;
					break;
				}
				reps[nrep++] = ci;
			}
			F.tapsel[s] = (int)q;
		}
		if (nrep) {
			if (first_rep < 0)
				first_rep = reps[0];
			if (nrep > 1 || !few ||
			    memcmp(t->chans[reps[0]].taps[0], t->chans[first_rep].taps[0], sizeof(float) * WR_FIR_LENGTH))
				g->one_filter = false;
		}
		if (!few || grp >= 64) {
			for (size_t s = base; s < base + WR_LANES; ++s)
				F.tapsel[s] = 0;
			if (nrep)
				g->uniform_taps = false;
			continue;
		}
		for (unsigned int q = 0; q < nrep; ++q)
			for (size_t j = 0; j < WR_LANES; ++j)               /* window order: sample j meets coeff[63 - j] */
				F.taps1u[(grp * WR_TAPSETS + q) * WR_LANES + j] = t->chans[reps[q]].taps[0][WR_FIR_LENGTH - 1 - j];
		g->nsets[grp] = (unsigned char)(nrep ? nrep : 1);
		g->fewsets_mask |= 1ull << grp;
		if (nrep <= 1)
			g->uniform_mask |= 1ull << grp;
		else
			g->uniform_taps = false;
	}
	g->one_filter = g->one_filter && first_rep >= 0;
	/* the audio filter likewise (one per lane group or the per-lane path; its taps go through the
	 * scalar cache, see post_role) */
	const unsigned int l2 = g->l2;
	const auto audio_taps = [l2](const Chan &c) { return l2 > WR_FIR_LENGTH ? c.taps_long2 : c.taps[1]; };
	F.taps2u.assign(S / WR_LANES * l2, 0.0f);
	for (size_t base = 0; base < S && base / WR_LANES < 64; base += WR_LANES) {
		bool same = true;
		const int rep = lane_group_rep(t, g, base, audio_taps, l2, &same);
		if (!same || rep < 0)
			continue;
		memcpy(&F.taps2u[base / WR_LANES * l2], audio_taps(t->chans[rep]), sizeof(float) * l2);
		g->uniform2_mask |= 1ull << (base / WR_LANES);
	}
	g->long_uniform = g->long_one = false;
	if (g->l1 > WR_FIR_LENGTH) {
		const auto long_taps = [](const Chan &c) { return c.taps_long; };
		g->long_uniform = g->long_one = true;
		int rep_all = -1;
		for (size_t base = 0; base < S && g->long_uniform; base += WR_LANES) {
			const int rep = lane_group_rep(t, g, base, long_taps, g->l1, &g->long_uniform);
			if (rep >= 0) {
				if (rep_all < 0)
					rep_all = rep;
				else if (memcmp(t->chans[rep].taps_long, t->chans[rep_all].taps_long, sizeof(float) * g->l1))
					g->long_one = false;
			}
		}
		g->long_one = g->long_one && g->long_uniform;
	}
	if (g->one_filter)
		/* two lane groups that share a wave take the window from the first one's entry: an emptied lane
		 * group in between holds the common filter too */
		for (size_t grp = 0; grp < S / WR_LANES; ++grp)
			for (size_t j = 0; j < WR_LANES; ++j)
				F.taps1u[(grp * WR_TAPSETS) * WR_LANES + j] = t->chans[first_rep].taps[0][WR_FIR_LENGTH - 1 - j];
}

/* push the host shadow of one group's parameters to its device arrays */
int wrc_group_upload(wr_tuner *t, Group *g)
{
	const size_t S = g->slots;
	hipStream_t st = t->dev->stream;
	if (int rc = wrc_tuner_quiesce(t))
		return rc;
	std::vector<unsigned int> step(S, 0);
	std::vector<int> flags(S, 0), mode(S, -1);      /* mode < 0 marks an idle slot */
	std::vector<float> taps1(S * WR_FIR_LENGTH, 0.0f), taps2(S * g->l2, 0.0f);
	std::vector<float> taps1b(g->d1b ? S * g->l1b : 0, 0.0f), gain(S, 1.0f), squelch(S, 0.0f);
	std::vector<float> taps1L(g->l1 > WR_FIR_LENGTH ? S * g->l1 : 0, 0.0f);
	std::vector<WrAgcPar> agc(S, WrAgcPar{0.0f, 0u, WR_AGC_IDLE, 1.0f});
	const unsigned int audio_rate = t->input_rate / g->d1 / (g->d1b ? g->d1b : 1u) / g->d2;
	g->use_gain = g->use_squelch = g->use_agc = false;
	for (size_t s = 0; s < S; ++s) {
		int ci = g->owner[s];
		if (ci < 0)
			continue;
		Chan &c = t->chans[ci];
		step[s] = c.stepL;
		mode[s] = c.mode;
		flags[s] = 1;
		for (int j = 0; j < WR_FIR_LENGTH; ++j)
			taps1[(size_t)j * S + s] = c.taps[0][j];
		for (unsigned int j = 0; j < g->l2; ++j)
			taps2[(size_t)j * S + s] = g->l2 > WR_FIR_LENGTH ? c.taps_long2[j] : c.taps[1][j];
		if (g->d1b)
			for (unsigned int j = 0; j < g->l1b; ++j)
				taps1b[(size_t)j * S + s] = g->l1b > WR_FIR_LENGTH ? c.taps_long1b[j] : c.taps[2][j];
		if (g->l1 > WR_FIR_LENGTH)
			for (unsigned int j = 0; j < g->l1; ++j)
				taps1L[(size_t)j * S + s] = c.taps_long[j];
		/* a channel with AGC: its af_gain follows the AGC (k_agc_rows), the post stage sees a gain of 1 */
		agc[s].step = WR_AGC_OFF;
		if (c.agc_on) {
			WrAgcPar &a = agc[s];
			if (wrd_agc_design(c.agc_dbfs, c.agc_decay, c.agc_max_gain, audio_rate, &a.target, &a.floor_bits, &a.step))
				return wrc_fail(WR_ERR_ARG, "AGC of channel %d: no step for an audio rate of %u Hz", ci, audio_rate);
			a.af_gain = c.gain;
			c.agc_used = a;
			g->use_agc = true;
		}
		c.agc_used_on = c.agc_on;
		gain[s] = c.agc_on ? 1.0f : c.gain;
		squelch[s] = c.squelch;
		g->use_gain = g->use_gain || gain[s] != 1.0f;
		g->use_squelch = g->use_squelch || c.squelch > 0.0f;
	}
	GroupFilters F;
	group_classify(t, g, F);
	/* per-slot turns of the ROTATE NCO (see WrGroupDev) */
	std::vector<float> rot(S * 4, 0.0f);
	{
		const float *turn = t->dev->turn_host;
		for (size_t s = 0; s < S; ++s) {
			const unsigned int Sx = step[s] >> 16;
			rot[4 * s + 0] = turn[(Sx + 16384u) & 0xFFFFu];
			rot[4 * s + 1] = turn[Sx & 0xFFFFu];
			rot[4 * s + 2] = turn[(Sx + 16385u) & 0xFFFFu];
			rot[4 * s + 3] = turn[(Sx + 1u) & 0xFFFFu];
		}
	}
	/* pageable sources: hipMemcpyAsync stages them before returning */
	HIP_TRY(hipMemcpyAsync(g->dev.step, step.data(), S * sizeof(unsigned int), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.flags, flags.data(), S * sizeof(int), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.mode, mode.data(), S * sizeof(int), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.taps1, taps1.data(), taps1.size() * sizeof(float), hipMemcpyHostToDevice, st));
	if (g->l1 > WR_FIR_LENGTH)
		HIP_TRY(hipMemcpyAsync(g->dev.taps1L, taps1L.data(), taps1L.size() * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.taps2, taps2.data(), taps2.size() * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.rot, rot.data(), rot.size() * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.taps1u, F.taps1u.data(), F.taps1u.size() * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.taps2u, F.taps2u.data(), F.taps2u.size() * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.tapsel, F.tapsel.data(), F.tapsel.size() * sizeof(int), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.gain, gain.data(), S * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(g->dev.squelch, squelch.data(), S * sizeof(float), hipMemcpyHostToDevice, st));
	if (g->d1b)
		HIP_TRY(hipMemcpyAsync(g->dev.taps1b, taps1b.data(), taps1b.size() * sizeof(float), hipMemcpyHostToDevice, st));
	if (g->use_agc)
		HIP_TRY(hipMemcpyAsync(g->agc_par, agc.data(), S * sizeof(WrAgcPar), hipMemcpyHostToDevice, st));
	/* what the setters staged for the channels themselves: phase, Demodulator prev_i/q, histories to be emptied */
	for (size_t s = 0; s < S; ++s) {
		int ci = g->owner[s];
		if (ci < 0)
			continue;
		Chan &c = t->chans[ci];
		if (c.phase_dirty) {
			HIP_TRY(hipMemcpyAsync(g->dev.phase[g->sp] + s, &c.phaseL, sizeof(unsigned int), hipMemcpyHostToDevice, st));
			c.phase_dirty = false;
			/* ROTATE keeps the turn INTO the next frame; a phase set from outside breaks that
			 * chain, so the channel filter starts from an empty history (see wr_chan_set_state) */
			if (t->nco_mode == WR_NCO_ROTATE)
				c.cs_hist_reset = true;
		}
		if (c.prev_dirty) {
			HIP_TRY(hipMemcpyAsync(g->dev.prev_iq[g->parity] + 2 * s, c.prev_iq, 2 * sizeof(float), hipMemcpyHostToDevice, st));
			c.prev_dirty = false;
		}
		if (c.cs_hist_reset) {
			/* 63 LO rows of this slot: one float2 per row, stride S float2 */
			HIP_TRY(hipMemset2DAsync(g->dev.hist_cs[g->sp] + 2 * s, S * 2 * sizeof(float), 0, 2 * sizeof(float),
			                         WR_HIST, st));
			HIP_TRY(hipMemset2DAsync(g->dev.hist_lo[g->sp] + 2 * s, S * 2 * sizeof(float), 0, 2 * sizeof(float),
			                         WR_HIST, st));
			HIP_TRY(hipMemset2DAsync(g->dev.iq2_hist[g->p2] + 2 * s, S * 2 * sizeof(float), 0, 2 * sizeof(float),
			                         g->l1b - 1, st));
			if (g->l1 > WR_FIR_LENGTH)        /* the L - 1 mixed frames of this slot */
				HIP_TRY(hipMemset2DAsync(g->dev.mixhist[g->sp] + 2 * s, S * 2 * sizeof(float), 0, 2 * sizeof(float),
				                         g->l1 - 1, st));
			c.cs_hist_reset = false;
		}
		if (c.dem_hist_reset) {
			/* 63 history rows of this slot: one float per row, stride S */
			HIP_TRY(hipMemset2DAsync(g->dev.dem[g->parity] + s, S * sizeof(float), 0, sizeof(float), g->l2 - 1, st));
			c.dem_hist_reset = false;
		}
		if (c.agc_on && c.agc_reset) {
			HIP_TRY(hipMemcpyAsync(g->agc_state + s, &c.agc_used.floor_bits, sizeof(unsigned int), hipMemcpyHostToDevice, st));
			c.agc_reset = false;
		}
	}
	HIP_TRY(hipStreamSynchronize(st));     /* host vectors go out of scope */
	g->dirty = false;
	return WR_OK;
}

/* fold recorded event pairs into the running mean once more than `keep` pairs are pending */
static int prof_drain(wr_tuner *t, size_t keep)
{
	if (t->ev_used / 2 <= keep)
		return WR_OK;
	HIP_TRY(wrc_dev_stream_sync(t->dev));
	for (size_t i = 0; i + 1 < t->ev_used; i += 2) {
		float ms = 0.0f;
		HIP_TRY(hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
		const unsigned int span = (i / 2 < t->ev_span.size() && t->ev_span[i / 2]) ? t->ev_span[i / 2] : 1u;
		t->prof_ms += ms;                           /* prof_ms / prof_n = mean per launch */
		t->prof_n += span;
	}
	t->ev_used = 0;
	t->ev_span.clear();
	return WR_OK;
}

/* room for one more event pair at t->ev[t->ev_used]: the pairs recorded so far are drained first, unless a group's
 * start event is still waiting for its stop (ev_used odd) */
static int prof_reserve_pair(wr_tuner *t)
{
	if (int rc = (t->ev_used & 1) ? WR_OK : prof_drain(t, 64))
		return rc;
	while (t->ev.size() < t->ev_used + 2) {
		hipEvent_t e;
		HIP_TRY(hipEventCreate(&e));
		t->ev.push_back(e);
	}
	return WR_OK;
}

/* the next event pair, for a launch that stamps its own start and stop; wrc_prof_pair_stamped when it has gone out */
int wrc_prof_pair_begin(wr_tuner *t, void **ev_start, void **ev_stop)
{
	if (int rc = prof_reserve_pair(t))
		return rc;
	*ev_start = t->ev[t->ev_used];
	*ev_stop = t->ev[t->ev_used + 1];
	return WR_OK;
}

void wrc_prof_pair_stamped(wr_tuner *t)
{
	t->ev_span.resize(t->ev_used / 2 + 1, 1u);
	t->ev_used += 2;
}

extern "C" int wr_tuner_profile(wr_tuner *t, int enable)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (int rc = wrc_settle_held(t))                    /* (a streaming launch stamps its events when it is opened) */
		return rc;
	if (t->ev_used & 1)
		t->ev_used--;                               /* a group left open: its start event is dropped */
	t->profiling = enable != 0;
	t->prof_stride = enable > 1 ? (unsigned int)enable : 1u;
	t->prof_tick = 0;
	return WR_OK;
}

extern "C" int wr_tuner_profile_read(wr_tuner *t, unsigned int *launches, double *mean_ms)
{
	if (!t || !launches || !mean_ms)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_profile_read: bad argument");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (int rc = wrc_settle_held(t))
		return rc;
	if (int rc = prof_drain(t, 0))
		return rc;
	*launches = t->prof_n;
	*mean_ms = t->prof_n ? t->prof_ms / t->prof_n : 0.0;
	t->prof_ms = 0.0;
	t->prof_n = 0;
	return WR_OK;
}

/* may this block wait for its successor?  Only whole audio frames: a block that is not a multiple
 * of every rate group's decimations restarts the decimation phase at its start (dspblock.cxx:177-178
 * truncates per block), which a merged block would not */
static bool block_can_be_held(const wr_tuner *t, size_t nframes)
{
	/* (nor a block of a tuner with an AGC on: its groups' post stages go out block by block) */
	for (const Chan &c : t->chans)
		if (c.in_use && c.agc_on)
			return false;
	for (const Group *g : t->groups) {
		if (g->active <= 0)
			continue;
		const size_t q = (size_t)g->d1 * (g->d1b ? g->d1b : 1u) * g->d2;
		if (!q || nframes % q)
			return false;
	}
	return true;
}

/* what a submit can be refused for before anything is enqueued -- checked before a block is HELD too,
 * so that a held wr_tuner_submit never returns WR_OK for a block a later call would have to refuse */
static int submit_precheck(const wr_tuner *t, size_t nframes, int where)
{
	if (nframes > t->max_block_frames)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_submit: %zu frames exceeds max_block_frames %zu", nframes,
		                t->max_block_frames);
	if (where != WR_HOST && where != WR_DEVICE)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_submit: bad `where`");
	for (const Chan &c : t->chans)
		if (c.in_use && c.group < 0)
			return wrc_fail(WR_ERR_STATE, "a channel has no filters (LowPass::init: \"Must specify either "
			                          "decimation or output rate\")");
	return WR_OK;
}

/* the host's mirror of the phase advance the kernels wrote into the other state set: `frames` input frames on
 * (downconverter.cxx:103), mod 2^32 */
void wrc_advance_phases(wr_tuner *t, unsigned long long frames)
{
	for (Chan &c : t->chans) {
		if (!c.in_use || c.group < 0)
			continue;
		c.phaseL += (unsigned int)frames * c.stepL;
	}
}

/* one submit on its way through the steps of wrc_tuner_submit_now */
struct Submit {
	const float *cur;            /* the block as the kernels read it: float IQ ... */
	const uint8_t *cur_u8;       /* ... or RTL-SDR bytes */
	size_t nframes;
	unsigned long long seq;
	/* stride 1: this submit's launch stamps its own start and stop (hipExtLaunchKernelGGL).  Stride
	 * n > 1: an event before the launch of the group's first submit and one after the launch of its
	 * last -- n launches and the gaps between them per pair, at 1/n of the events' own cost. */
	bool prof_now, group_first, group_last;
	bool hist_written = false;
	bool marked = false, unmarked = false;   /* wr_tuner_mark_launches: launches that stamped the submit's event / that could not */
};

/* a WR_HOST block comes over into t->in_stage, sparsely or whole; `*u8`: what the staged block holds */
static int submit_stage_host(wr_tuner *t, const void *iq, size_t nframes, bool *u8)
{
	wr_dev *d = t->dev;
	hipStream_t st = d->stream;
	if (!t->in_stage)
		HIP_TRY(hipMalloc((void **)&t->in_stage, t->max_block_frames * 2 * sizeof(float)));
	/* r04: a block in PAGE-LOCKED host memory whose receivers all read it through sparse windows of one shape -- the same
	 * decimation, the same channel-filter length, a window at most every second filter length -- never crosses PCIe
	 * whole: the staging kernel brings over the frames under the taps and the tail (wr_stage_windows_from_host says
	 * which), as floats whatever the source format.  Pageable memory, mixed shapes, dense windows: the copy, as before. */
	bool sparse = false;
	if (nframes && !(((uintptr_t)iq | (uintptr_t)t->in_stage) & 15u)) {
		unsigned int sd = 0, sl = 0;
		bool same = true;
		for (const Group *g : t->groups) {
			if (g->active <= 0)
				continue;
			if (!sd) {
				sd = g->d1;
				sl = g->l1;
			} else if (g->d1 != sd || g->l1 != sl) {
				same = false;
			}
		}
		void *mapped = nullptr;
		if (same && sd && sd >= 2u * sl && nframes >= 4u * (size_t)sd) {
			/* is the block page-locked?  Asked once per buffer: the same source comes back block after block, and for a
			 * pageable one the question is a failing runtime call every time.  Only the probe's OWN error is cleared
			 * (a blanket hipGetLastError() here could swallow the pending error of an earlier asynchronous launch) */
			if (iq != t->probe_ptr || t->probe_gen != d->reg_gen || !t->probe_left--) {
				mapped = wrc_host_mapped(iq);
				if (!mapped) {
					t->probe_ptr = iq;                  /* pageable: remembered until something is page-locked or released
					                                       through this library (a "yes" is asked again every time: it is cheap,
					                                       and an address that is no longer mapped must never be used) */
					t->probe_gen = d->reg_gen;
					t->probe_left = 64;                 /* (... or until 64 blocks later: the application may page-lock it itself) */
				}
			}
		}
		if (mapped) {
			HIP_TRY(wrk_stage_windows(st, mapped, *u8, t->in_stage, nframes, sd, sl, sl - 1u));
			if (int rc = wrc_upload_mark(d, st))            /* (wr_dev_wait_uploads: the kernel has read the host block) */
				return rc;
			sparse = true;
		}
	}
	if (nframes && !sparse)
		HIP_TRY(hipMemcpyAsync(t->in_stage, iq, nframes * 2 * (*u8 ? sizeof(uint8_t) : sizeof(float)),
		                       hipMemcpyHostToDevice, st));
	t->last_staging = sparse ? 2 : 1;
	if (sparse)
		*u8 = false;                         /* the staged block holds floats */
	return WR_OK;
}

/* demodulator output wanted (wr_tuner_keep_stages) or an unusual audio decimation: demod
 * and audio filter as two kernels with the demod rows in HBM, at once.  Otherwise one
 * fused pass -- deferred to the next launch where that launch can carry it. */
static int submit_post(wr_tuner *t, Group *g, const Submit &S, const WrTunerLaunch &L, const WrTunerLaunch &Lp,
                       const WrGroupDev &Gp, bool two_kernels)
{
	hipStream_t st = t->dev->stream;
	/* (r04: a group with a long channel filter defers too where its launch can carry a post stage: the ROTATE kernel,
	 * every lane group on one long filter) */
	const bool long_rides = g->l1 > WR_FIR_LENGTH && g->long_uniform;
	/* (r05: an audio filter of 128 / 256 taps -- k_tuner_post<D2, 2 | 4> -- goes out on its own behind the DDC: the
	 * workgroups that ride are compiled for 64 taps) */
	/* (r05: a group with a second channel stage defers as well -- its post stage reads chan_iq2, which the NEXT block's
	 * k_tuner_iq2 does not touch: that one writes the other buffer, behind the launch the post stage rides in) */
	/* (a group with an AGC on does not defer: k_agc_rows follows the post stage on the group's audio, below) */
	const bool defer = !two_kernels && (g->l1 <= WR_FIR_LENGTH || long_rides) && Lp.k1 && t->defer_post &&
	                   t->nco_mode == WR_NCO_ROTATE && g->l2 == WR_FIR_LENGTH && !g->use_agc;
	WrTunerLaunch Lq = Lp;
	if (g->use_agc)
		Lq.audio_scale = 1.0f;                  /* the sink's scale comes behind the AGC: k_agc_rows applies it to every slot in use */
	if (two_kernels) {
		HIP_TRY(wrk_tuner_demod(st, Lq, Gp));
		HIP_TRY(wrk_tuner_audio(st, Lq, Gp));
	} else if (defer) {
		g->post_pending = true;
		g->post_args = wrk_post_args(Lp, Gp);
		g->pend_seq = S.seq;
		g->pend_k2 = Lp.k2;
		g->pend_slots = L.slots_used;
		g->post_args.audio_host = wrc_ring_reserve(t, g, Lp.k2, L.slots_used);
		g->post_args.host_stride = Lp.k2;           /* the ring's rows lie back to back (RingSlot::stride = frames) */
		g->pend_direct = g->post_args.audio_host != nullptr;
	} else {
		HIP_TRY(wrk_tuner_post(st, Lq, Gp));
	}
	if (g->use_agc && Lp.k2) {
		/* whichever way the audio was made: in place, before the ring's copy (and every getter) reads it */
		HIP_TRY(wrk_agc_rows(st, g->dev.audio, g->k2max, L.slots_used, Lp.k2, g->agc_par, g->agc_state, t->audio_scale));
		++t->agc_launches;
	}
	if (!defer)
		return wrc_ring_push(t, g, S.seq, Lp.k2, L.slots_used, false);
	return WR_OK;
}

/* one rate group's block: a pending seek, the DDC, the second channel stage, the post stage; then its indices roll */
static int submit_group(wr_tuner *t, Group *g, Submit &S)
{
	wr_dev *d = t->dev;
	hipStream_t st = d->stream;
	if (g->dirty)
		if (int rc = wrc_group_upload(t, g))
			return rc;
	WrTunerLaunch L = wrc_group_launch(t, g, S.cur, S.cur_u8, S.nframes);
	/* the events this launch stamps or is bracketed by: the profiler's, or the submit's completion mark */
	if (S.group_first)
		if (int rc = prof_reserve_pair(t))
			return rc;
	if (S.prof_now) {
		/* stamped by the launch itself (wrk_tuner_ddc) */
		if (int rc = wrc_prof_pair_begin(t, &L.ev_start, &L.ev_stop))
			return rc;
		if (t->mark_launches)
			S.unmarked = true;              /* the launch's stop event is the profiler's: the completion mark is an
			                                   ordinary record behind it (below) */
	} else if (t->mark_launches && g->l1 <= WR_FIR_LENGTH) {
		L.ev_start = nullptr;               /* completion only: the slot of this submit (every rate group's launch
		                                       stamps it in turn: the last one stands) */
		L.ev_stop = t->launch_ev[(t->launches_marked + 1) % 4];
		S.marked = true;
	} else if (t->mark_launches) {
		S.unmarked = true;
	}
	if (S.group_first && !(t->ev_used & 1)) {
		/* (once per submit: the first rate group's launch is the first of the bracket) */
		HIP_TRY(hipEventRecord(t->ev[t->ev_used], st));
		t->ev_used += 1;
	}
	/* a seek that is still pending (wr_tuner_seek): this launch takes the phase in closed form and reads the
	 * all-zero state sets; with the demodulator rows kept (two kernels) it is made real first */
	const bool two_kernels = (t->keep_mask & (1u << WR_STAGE_DEMOD)) != 0 || !wrk_tuner_post_supported(L.d2);
	WrGroupDev Gs = g->dev;
	if (g->seek_pending) {
		if (two_kernels || g->d1b || g->l1 > WR_FIR_LENGTH) {
			if (g->post_pending)
				if (int rc = wrc_post_send_pending(t, g, false))
					return rc;
			if (int rc = wrc_seek_materialize(t, g))
				return rc;
		} else {
			L.seeking = true;
			L.seek_lo = (unsigned int)g->seek_frame;
			Gs.hist_cs[g->sp] = g->z_hist;
			Gs.hist_lo[g->sp] = g->z_hist;
			Gs.prev_iq[g->parity] = g->z_prev;
			Gs.dem[g->parity] = g->z_dem;
			g->seek_pending = false;
		}
	}
	/* The previous block's post stage rides along with this block's DDC where the kernel
	 * variant can take it (wrk_tuner_ddc says); otherwise it goes out on its own first. */
	bool rode = false;
	if (g->l1 > WR_FIR_LENGTH)
		/* a channel filter of 128 or 256 taps: the plain kernel with the reference's arithmetic (wr_kernels.hip:
		 * k_tuner_ddc_long), which also rolls phase and mixed history; r04: its ROTATE form carries the previous block's post stage like the 64-tap kernel */
		HIP_TRY(wrk_tuner_ddc_long(st, L, g->dev, g->l1, d->table, d->num_cus,
		                           t->nco_mode != WR_NCO_EXACT && g->long_uniform, g->long_one, d->hi_cs, d->lo_cs,
		                           g->post_pending ? &g->post_args : nullptr, &rode));
	else
		HIP_TRY(wrk_tuner_ddc(st, L, Gs, t->nco_mode == WR_NCO_ROTATE ? d->table_turn : d->table, d->hi_cs, d->lo_cs,
		                      d->num_cus, g->post_pending ? &g->post_args : nullptr, &rode));
	if (S.prof_now)
		wrc_prof_pair_stamped(t);
	if (g->post_pending)
		if (int rc = wrc_post_send_pending(t, g, rode))
			return rc;
	/* A second channel-filter stage sits between the DDC and the demodulator: its kernel runs
	 * here, and everything after it works on ITS output (chan_iq2) at ITS rate. */
	WrTunerLaunch Lp = L;
	WrGroupDev Gp = Gs;
	if (g->d1b) {
		HIP_TRY(wrk_tuner_iq2(st, g->dev, g->slots, L.slots_used, L.k1, g->d1b, g->cb, g->p2));
		g->p2 ^= 1;
		Lp.k1 = L.k1 / g->d1b;
		Lp.k2 = Lp.k1 / g->d2;
		Gp.chan_iq[0] = g->dev.chan_iq2[0];
		Gp.chan_iq[1] = g->dev.chan_iq2[1];
	}
	if (int rc = submit_post(t, g, S, L, Lp, Gp, two_kernels))
		return rc;
	g->last_demod_kept = two_kernels;
	g->last_parity = g->parity;
	g->last_cb = g->cb;
	g->sp ^= 1;                    /* the kernels wrote the other state set */
	if (g->l1 <= WR_FIR_LENGTH)
		S.hist_written = true;     /* k_tuner_ddc stored the next input history (k_tuner_ddc_long keeps its own) */
	if (Lp.k1)
		g->parity ^= 1;            /* k_tuner_demod filled the other prev_iq / dem history */
	if (L.k1)
		g->cb ^= 1;
	g->last_k1 = Lp.k1;            /* frames at the demodulator's input */
	g->last_k2 = Lp.k2;
	return WR_OK;
}

/* the bracket of a profiling stride closes behind the LAST rate group's launches of its last submit
 * (it used to close behind the first group's: the others' launches were credited and not timed) */
static int submit_prof_close(wr_tuner *t, const Submit &S)
{
	if (S.group_last && (t->ev_used & 1)) {
		HIP_TRY(hipEventRecord(t->ev[t->ev_used], t->dev->stream));
		t->ev_span.resize(t->ev_used / 2 + 1, 1u);
		t->ev_span[t->ev_used / 2] = t->prof_stride;
		t->ev_used += 1;
	}
	return WR_OK;
}

/* the last 63 frames of the block for the next one, where no DDC launch has stored them */
static int submit_input_hist(wr_tuner *t, const Submit &S)
{
	if (!S.hist_written)
		HIP_TRY(wrk_input_hist(t->dev->stream, S.cur, S.cur_u8, S.nframes, t->in_hist[t->in_par], t->in_hist[t->in_par ^ 1]));
	t->in_par ^= 1;
	return WR_OK;
}

/* wr_tuner_mark_launches: the submit's completion mark, where no launch could stamp it */
static int submit_launch_mark(wr_tuner *t, Submit &S)
{
	if (t->mark_launches && !S.marked && !S.unmarked && S.nframes)
		S.unmarked = true;                          /* (no rate group launched anything, but k_input_hist above reads the block: the
		                                               completion mark must not be the block-before's -- a halo exchange ordered
		                                               behind it could overwrite what that kernel is still reading) */
	if (t->mark_launches && (S.marked || S.unmarked)) {
		/* (a launch that could not stamp it -- profiling, a long channel filter -- or a history kernel behind the DDC:
		 * an ordinary record, at an ordinary record's price) */
		if (S.unmarked || !S.hist_written)
			HIP_TRY(hipEventRecord(t->launch_ev[(t->launches_marked + 1) % 4], t->dev->stream));
		++t->launches_marked;
	}
	return WR_OK;
}

int wrc_tuner_submit_now(wr_tuner *t, const void *iq, size_t nframes, int where, bool u8)
{
	if (!t || (nframes && !iq))
		return wrc_fail(WR_ERR_ARG, "wr_tuner_submit: bad argument");
	if (int rc = submit_precheck(t, nframes, where))
		return rc;
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;

	const void *src = iq;
	if (where == WR_HOST) {
		if (int rc = submit_stage_host(t, iq, nframes, &u8))
			return rc;
		src = t->in_stage;
	}
	t->stream.last_iq = nullptr;             /* (the last block's channel IQ is in the group's own buffers again) */
	Submit S;
	S.cur = u8 ? nullptr : (const float *)src;
	S.cur_u8 = u8 ? (const uint8_t *)src : nullptr;
	S.nframes = nframes;
	S.seq = t->submit_seq++;
	const unsigned int prof_pos = t->profiling ? t->prof_tick++ % t->prof_stride : 0u;
	S.prof_now = t->profiling && t->prof_stride == 1;
	S.group_first = t->profiling && t->prof_stride > 1 && prof_pos == 0;
	S.group_last = t->profiling && t->prof_stride > 1 && prof_pos == t->prof_stride - 1 && (t->ev_used & 1);
	for (Group *g : t->groups) {
		if (g->active <= 0) {
			g->last_k1 = g->last_k2 = 0;
			continue;
		}
		if (int rc = submit_group(t, g, S))
			return rc;
	}
	if (int rc = submit_prof_close(t, S))
		return rc;
	if (int rc = submit_input_hist(t, S))
		return rc;
	if (int rc = submit_launch_mark(t, S))
		return rc;

	wrc_advance_phases(t, nframes);
	t->submitted = true;
	return WR_OK;
}

int wrc_tuner_launch_held(wr_tuner *t)
{
	if (t->stream.live)                                 /* (a streaming launch holds no blocks back: it is told that none follows) */
		return wrc_stream_close(t);
	if (!t->held_count)
		return WR_OK;
	const float *base = t->held_base;
	const size_t frames = t->held_frames;
	t->held_count = 0;
	t->held_base = nullptr;
	t->held_frames = 0;
	return wrc_tuner_submit_now(t, base, frames, WR_DEVICE, false);
}

static int tuner_submit(wr_tuner *t, const void *iq, size_t nframes, int where, bool u8)
{
	if (!t || (nframes && !iq))
		return wrc_fail(WR_ERR_ARG, "wr_tuner_submit: bad argument");
	if (int rc = submit_precheck(t, nframes, where))
		return rc;
	if (t->stream.live) {
		if (wrc_stream_follows(t, nframes, where, u8))
			return wrc_stream_bell(t, iq, false);
		if (!(t->stream.ext && where == WR_HOST && u8 && wrc_stream_follows(t, nframes, WR_DEVICE, true)))
			if (int rc = wrc_stream_close(t))
				return rc;
	}
	if (t->stream.enabled && where == WR_DEVICE && nframes) {
		bool took = false;
		t->stream.ext = false;
		const int rc = wrc_stream_open(t, iq, nframes, u8, &took);
		if (rc || took)
			return rc;
	}
	if (t->stream.enabled && t->stream.host_bytes && where == WR_HOST && u8 && nframes) {
		bool took = false;
		const int rc = wrc_stream_host_u8(t, (const uint8_t *)iq, nframes, &took);
		if (rc || took)
			return rc;
	}
	if (t->coalesce > 1 && where == WR_DEVICE && !u8 && nframes && block_can_be_held(t, nframes)) {
		const float *p = (const float *)iq;
		/* (a setter called since the last submit has sent the held blocks out already: wrc_settle_held) */
		const bool follows = t->held_count && p == t->held_base + 2 * t->held_frames &&
		                     nframes == t->held_each && t->held_frames + nframes <= t->max_block_frames;
		if (!follows) {
			if (int rc = wrc_tuner_launch_held(t))
				return rc;
			if (nframes * 2 > t->max_block_frames)          /* no room for a second one: nothing to wait for */
				return wrc_tuner_submit_now(t, iq, nframes, where, u8);
			t->held_base = p;
			t->held_frames = 0;
			t->held_each = nframes;
		}
		t->held_frames += nframes;
		t->held_count++;
		if (t->held_count >= t->coalesce || t->held_frames + nframes > t->max_block_frames)
			return wrc_tuner_launch_held(t);
		return WR_OK;
	}
	if (int rc = wrc_tuner_launch_held(t))                      /* keep the stream in order */
		return rc;
	return wrc_tuner_submit_now(t, iq, nframes, where, u8);
}

extern "C" int wr_tuner_submit(wr_tuner *t, const float *iq, size_t nframes, int where)
{
	return tuner_submit(t, iq, nframes, where, false);
}

extern "C" int wr_tuner_submit_u8(wr_tuner *t, const uint8_t *iq_u8, size_t nframes, int where)
{
	return tuner_submit(t, iq_u8, nframes, where, true);
}

extern "C" int wr_tuner_last_staging(wr_tuner *t, int *how)
{
	if (!t || !how)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_last_staging: bad argument");
	*how = t->last_staging;
	return WR_OK;
}

extern "C" int wr_tuner_set_blocks_per_launch(wr_tuner *t, unsigned int nblocks)
{
	if (!t || !nblocks)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_set_blocks_per_launch: bad argument");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_launch_held(t))
		return rc;
	t->coalesce = nblocks;
	return WR_OK;
}

extern "C" int wr_tuner_submit_count(wr_tuner *t, unsigned long long *submits)
{
	if (!t || !submits)
		return wrc_fail(WR_ERR_ARG, "tuner or submits is NULL");
	*submits = t->submit_seq;                /* (written by submits only: call from the thread that submits) */
	return WR_OK;
}

extern "C" int wr_tuner_mark_launches(wr_tuner *t, int enable)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (enable)
		for (int i = 0; i < 4; ++i)
			if (!t->launch_ev[i])
				HIP_TRY(hipEventCreateWithFlags(&t->launch_ev[i], hipEventDisableTiming | hipEventReleaseToDevice));
	if (enable && !t->mark_launches) {
		/* blocks launched before marking was on carry no mark: one ordinary record behind them (and behind the held
		 * ones, which go out now) stands for all of them */
		if (int rc = wrc_tuner_launch_held(t))
			return rc;
		if (t->submitted) {
			HIP_TRY(hipEventRecord(t->launch_ev[(t->launches_marked + 1) % 4], t->dev->stream));
			++t->launches_marked;
		}
	}
	t->mark_launches = enable != 0;
	return WR_OK;
}

/* wr_ring_exchange_after: the event that fires when every block submitted to `t` so far has been read (*ev = nullptr:
 * the tuner has launched nothing yet, nothing to wait for).  Blocks still held by wr_tuner_set_blocks_per_launch are
 * launched first; a tuner that does not mark its launches is an error, not a silent "no ordering". */
int wrc_tuner_launch_mark(wr_tuner *t, hipEvent_t *ev)
{
	*ev = nullptr;
	if (!t->mark_launches)
		return wrc_fail(WR_ERR_STATE, "wr_ring_exchange_after: wr_tuner_mark_launches(tuner, 1) first");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_launch_held(t))
		return rc;
	if (t->launches_marked)
		*ev = t->launch_ev[t->launches_marked % 4];
	return WR_OK;
}
