/*
 * wr_tuner.hip -- the tuner of the extern "C" boundary declared in include/webradio_amd.h: channels, rate groups,
 * staged parameter updates, launch sequencing (submit, flush, fetch, seek), profiling and launch marks.  No DSP
 * arithmetic lives here (design math: wr_design.cpp; kernels: wr_kernels.hip).  The host half of the streaming launch
 * is in wr_tuner_stream.hip, the pinned audio ring in wr_tuner_ring.hip.
 */
#include "wr_capi_internal.h"

static int dev_alloc_zero(void **p, size_t count, size_t elem)
{
	HIP_TRY(hipMalloc(p, (count ? count : 1) * elem));
	HIP_TRY(hipMemset(*p, 0, (count ? count : 1) * elem));
	/* (the fill is ordered on the null stream; a context on a non-blocking stream of its own -- WR_STREAM_PRIVATE --
	 * is not ordered behind it: wait here, this is set-up code) */
	HIP_TRY(hipStreamSynchronize(nullptr));
	return WR_OK;
}

/* ------------------------------------------------------------------ tuner -- */

/* lane groups that hold at least one channel: [0, used) in units of slots */
unsigned int wrc_group_slots_used(const Group *g)
{
	unsigned int hi = 0;
	for (unsigned int s = 0; s < g->slots; ++s)
		if (g->owner[s] >= 0)
			hi = s + 1;
	return ((hi + WR_LANES - 1) / WR_LANES) * WR_LANES;
}

/* a rate group's view for the kernels of one block of `nframes` frames at `cur` (float IQ) or `cur_u8` (RTL-SDR bytes):
 * what wrc_tuner_submit_now hands k_tuner_ddc and the post stage, and wrc_stream_open the streaming launch.  No events. */
WrTunerLaunch wrc_group_launch(const wr_tuner *t, const Group *g, const float *cur, const uint8_t *cur_u8,
                               size_t nframes)
{
	WrTunerLaunch L;
	L.cur = cur;
	L.cur_u8 = cur_u8;
	L.hist = t->in_hist[t->in_par];
	L.hist_next = t->in_hist[t->in_par ^ 1];
	L.parity = g->parity;
	L.sp = g->sp;
	L.cb = g->cb;
	L.nframes = nframes;
	L.d1 = g->d1;
	L.d2 = g->d2;
	L.slots = g->slots;
	L.slots_used = wrc_group_slots_used(g);
	L.k1 = nframes / g->d1;                 /* dspblock.cxx:177-178 */
	L.k2 = L.k1 / g->d2;
	L.k2max = g->k2max;
	L.nco_mode = t->nco_mode;
	L.uniform_mask = g->uniform_mask;
	L.uniform2_mask = g->uniform2_mask;
	L.fewsets_mask = g->fewsets_mask;
	L.one_filter = g->one_filter ? 1 : 0;
	memcpy(L.nsets, g->nsets, sizeof(L.nsets));
	L.audio_scale = t->audio_scale;
	L.use_gain = g->use_gain ? 1 : 0;
	L.use_squelch = g->use_squelch ? 1 : 0;
	L.ev_start = L.ev_stop = nullptr;
	return L;
}

/* a rate group's device arrays, each with its length in elements: what group_create allocates (in this order) and
 * group_free releases.  Built from the group's shape: a group without a long channel filter or a second channel
 * stage has no arrays for them. */
struct GroupArray {
	void **p;
	size_t count, elem;
};
static std::vector<GroupArray> group_arrays(Group *g)
{
	const size_t S = g->slots;
	const unsigned int l1 = g->l1, d1b = g->d1b;
	WrGroupDev &D = g->dev;
	std::vector<GroupArray> a;
	auto add = [&a](auto **p, size_t count) { a.push_back({(void **)p, count, sizeof(**p)}); };
	auto add2 = [&add](auto &pair, size_t count) { add(&pair[0], count); add(&pair[1], count); };   /* a ping-pong pair */
	add2(D.phase, S);
	add(&D.step, S);
	add2(D.hist_cs, (size_t)WR_HIST * S * 2);
	add2(D.hist_lo, (size_t)WR_HIST * S * 2);
	add(&D.flags, S);
	add(&D.mode, S);
	add(&D.taps1, S * WR_FIR_LENGTH);
	add(&D.taps2, S * g->l2);
	add(&D.rot, S * 4);
	add(&D.taps1u, S * WR_TAPSETS);
	add(&D.taps2u, S / WR_LANES * g->l2);      /* [lane groups][l2] */
	add(&D.tapsel, S);
	if (l1 > WR_FIR_LENGTH) {
		add(&D.taps1L, S * l1);
		add2(D.mixhist, (size_t)(l1 - 1) * S * 2);
	}
	add(&D.gain, S);
	add(&D.squelch, S);
	add2(D.iq2_hist, (size_t)(g->l1b - 1) * S * 2);         /* wr_tuner_seek clears it */
	if (d1b) {
		add(&D.taps1b, S * g->l1b);
		add2(D.chan_iq2, (g->k1max / d1b + 1) * S * 2);
	}
	add(&g->z_hist, (size_t)WR_HIST * S * 2);
	add(&g->z_prev, S * 2);
	add(&g->z_dem, (size_t)(g->l2 - 1) * S);
	add(&g->agc_par, S);
	add(&g->agc_state, S);
	add2(D.prev_iq, S * 2);
	add2(D.chan_iq, (g->k1max ? g->k1max : 1) * S * 2);
	add2(D.dem, ((size_t)g->l2 - 1 + g->k1max) * S);
	for (float *&audio : D.audio_set)
		add(&audio, g->k2max * S);                      /* (`audio` is one of them) */
	return a;
}

static void group_free(Group *g)
{
	if (!g)
		return;
	for (const GroupArray &a : group_arrays(g))
		(void)hipFree(*a.p);
	delete g;
}

static int group_create(wr_tuner *t, unsigned int d1, unsigned int d1b, unsigned int d2, unsigned int l1, unsigned int l1b,
                        unsigned int l2, Group **out)
{
	Group *g = new (std::nothrow) Group();
	if (!g)
		return wrc_fail(WR_ERR_NOMEM, "out of memory");
	memset(&g->dev, 0, sizeof(g->dev));
	g->parity = g->last_parity = 0;
	g->sp = g->cb = g->last_cb = 0;
	g->d1 = d1;
	g->d1b = d1b;
	g->d2 = d2;
	g->l1 = l1;
	g->l2 = l2;
	g->l1b = d1b ? l1b : (unsigned int)WR_FIR_LENGTH;
	g->slots = ((t->max_channels + WR_LANES - 1) / WR_LANES) * WR_LANES;
	g->k1max = t->max_block_frames / d1;       /* first-stage frames; the later stages need no more */
	g->k2max = g->k1max / (d1b ? d1b : 1u) / d2;
	if (g->k2max == 0)
		g->k2max = 1;
	g->owner.assign(g->slots, -1);
	g->dirty = true;
	g->uniform_taps = false;
	g->last_k1 = g->last_k2 = 0;
	g->active = 0;
	g->dev.l2 = g->l2;
	g->dev.l1b = g->l1b;
	int rc = WR_OK;
	for (const GroupArray &a : group_arrays(g))
		if ((rc = dev_alloc_zero(a.p, a.count, a.elem)) != WR_OK)
			break;
	g->dev.audio = g->dev.audio_set[0];
	g->audio_cur = 0;
	if (rc) {
		group_free(g);
		return rc;
	}
	*out = g;
	return WR_OK;
}

extern "C" int wr_tuner_create(wr_tuner **tuner, wr_dev *dev, unsigned int input_rate,
                               unsigned int max_channels, size_t max_block_frames, int nco_mode)
{
	if (!tuner || !dev || !input_rate || !max_channels || !max_block_frames)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_create: bad argument");
	if (nco_mode != WR_NCO_SPLIT && nco_mode != WR_NCO_EXACT && nco_mode != WR_NCO_ROTATE)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_create: bad nco_mode %d", nco_mode);
	if (max_channels > WR_MAX_CHANNELS)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_create: %u channels, at most %u per tuner (64 lane groups of 64)",
		                max_channels, (unsigned)WR_MAX_CHANNELS);
	*tuner = nullptr;
	if (wrc_dev_bind(dev))
		return WR_ERR_HIP;
	DEV_SETTLE(dev);                                        /* (the allocations below fill through the null stream and wait for it) */
	wr_tuner *t = new (std::nothrow) wr_tuner();
	if (!t)
		return wrc_fail(WR_ERR_NOMEM, "out of memory");
	t->dev = dev;
	t->input_rate = input_rate;
	t->max_channels = max_channels;
	t->max_block_frames = max_block_frames;
	t->nco_mode = nco_mode;
	t->keep_mask = 0;
	t->in_stage = nullptr;
	t->in_hist[0] = t->in_hist[1] = nullptr;
	t->in_par = 0;
	t->submitted = false;
	t->audio_scale = 1.0f;
	{
		const char *e = getenv("WR_DEFER_POST");
		t->defer_post = !(e && *e == '0');
	}
	t->profiling = false;
	t->prof_stride = 1;
	t->prof_tick = 0;
	t->ev_used = 0;
	t->prof_ms = 0.0;
	t->prof_n = 0;
	int rc = dev_alloc_zero((void **)&t->in_hist[0], (size_t)WR_HIST * 2, sizeof(float));
	if (!rc)
		rc = dev_alloc_zero((void **)&t->in_hist[1], (size_t)WR_HIST * 2, sizeof(float));
	if (rc) {
		wr_tuner_destroy(t);
		return rc;
	}
	*tuner = t;
	return WR_OK;
}

extern "C" int wr_tuner_destroy(wr_tuner *t)
{
	if (!t)
		return WR_OK;
	(void)hipSetDevice(t->dev->device);
	(void)wrc_stream_close(t);
	(void)wrc_dev_stream_sync(t->dev);
	wrc_stream_free(t);
	for (Group *g : t->groups)
		group_free(g);
	for (hipEvent_t e : t->ev)
		(void)hipEventDestroy(e);
	for (hipEvent_t e : t->launch_ev)
		if (e)
			(void)hipEventDestroy(e);
	for (wr_tuner::RingSlot &r : t->ring) {
		if (r.done)
			(void)hipEventDestroy(r.done);
		(void)hipHostFree(r.host);
	}
	(void)hipFree(t->in_stage);
	(void)hipFree(t->in_hist[0]);
	(void)hipFree(t->in_hist[1]);
	delete t;
	return WR_OK;
}

/* the tuner's one active rate group, or NULL: there is none, or (`*several`) more than one */
Group *wrc_single_group(wr_tuner *t, bool *several)
{
	Group *g = nullptr;
	unsigned int active = 0;
	for (Group *x : t->groups)
		if (x->active > 0 && ++active == 1)
			g = x;
	if (several)
		*several = active > 1;
	return active == 1 ? g : nullptr;
}

/* the pending post stage of a group goes out -- unless it `rode` in a launch already -- and its block is queued */
static int post_send_pending(wr_tuner *t, Group *g, bool rode)
{
	if (!rode)
		HIP_TRY(wrk_tuner_post_args(t->dev->stream, g->post_args));
	g->post_pending = false;
	return wrc_ring_push(t, g, g->pend_seq, g->pend_k2, g->pend_slots, g->pend_direct);
}

/* launch whatever post stage is still pending (results of the last submit wanted now) */
int wrc_tuner_flush(wr_tuner *t)
{
	{
		int rc = wrc_tuner_launch_held(t);
		if (rc)
			return rc;
	}
	for (Group *g : t->groups) {
		if (!g->post_pending)
			continue;
		if (int rc = post_send_pending(t, g, false))
			return rc;
	}
	return WR_OK;
}

static int seek_materialize(wr_tuner *t, Group *g)
{
	if (!g->seek_pending)
		return WR_OK;
	/* (a post stage still waiting for the next submit would write ITS end-of-block state over the seek's: the caller
	 * has flushed) */
	g->seek_pending = false;
	HIP_TRY(wrk_seek(t->dev->stream, g->dev, (unsigned int)g->slots, g->sp, g->parity, g->p2, g->seek_frame));
	return WR_OK;
}

/* host is about to touch device arrays the kernels of the last submit read or write: get the
 * pending post stage out, then drain the stream */
int wrc_tuner_quiesce(wr_tuner *t)
{
	int rc = wrc_tuner_flush(t);
	if (rc)
		return rc;
	for (Group *g : t->groups)
		if ((rc = seek_materialize(t, g)) != WR_OK)
			return rc;
	HIP_TRY(wrc_dev_stream_sync(t->dev));
	return wrc_stream_check(t);
}

/* Blocks waiting for their successors (wr_tuner_set_blocks_per_launch) go out before anything is
 * staged or read: a setter takes effect at the boundary after the last block SUBMITTED, and a
 * getter sees the state after it. */
int wrc_settle_held(wr_tuner *t)
{
	if (!t || (!t->held_count && !t->stream.live))
		return WR_OK;
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	return wrc_tuner_launch_held(t);
}

/* why the last chan_get() of this thread returned no channel: the error of sending the held blocks
 * out (already in wr_last_error()), or WR_OK when there simply is no such channel */
static thread_local int g_settle_rc = WR_OK;

static Chan *chan_get(wr_tuner *t, int chan)
{
	g_settle_rc = wrc_settle_held(t);
	if (g_settle_rc)
		return nullptr;
	if (!t || chan < 0 || (size_t)chan >= t->chans.size() || !t->chans[chan].in_use)
		return nullptr;
	return &t->chans[chan];
}

static int chans_live(const wr_tuner *t)
{
	int live = 0;
	for (const Chan &c : t->chans)
		live += c.in_use ? 1 : 0;
	return live;
}

extern "C" int wr_chan_add(wr_tuner *t, int *chan)
{
	if (!t || !chan)
		return wrc_fail(WR_ERR_ARG, "wr_chan_add: bad argument");
	if (int rc = wrc_settle_held(t))
		return rc;
	if ((unsigned int)chans_live(t) >= t->max_channels)
		return wrc_fail(WR_ERR_STATE, "wr_chan_add: tuner already has %u channels", t->max_channels);
	int idx = -1;
	for (size_t i = 0; i < t->chans.size(); ++i)
		if (!t->chans[i].in_use) {
			idx = (int)i;
			break;
		}
	if (idx < 0) {
		t->chans.push_back(Chan());
		idx = (int)t->chans.size() - 1;
	}
	Chan &c = t->chans[idx];
	memset(&c, 0, sizeof(c));
	c.in_use = true;
	c.len1 = c.len2 = c.len1b = WR_FIR_LENGTH;
	c.mode = WR_AM;                /* Demodulator ctor, demodulator.cxx:34 */
	c.gain = 1.0f;                 /* what the reference reports: af_gain 0, squelch_threshold 0 (receiverhandler.cxx:118-119) */
	c.squelch = 0.0f;
	c.group = -1;
	c.slot = -1;
	*chan = idx;
	return WR_OK;
}

/* take a channel out of its group slot; optionally keep Demodulator prev_i/q
 * (they survive stop()/start() in the reference, quirk Q5) */
static int chan_unseat(wr_tuner *t, Chan &c, bool keep_state)
{
	if (c.group < 0)
		return WR_OK;
	Group *g = t->groups[c.group];
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	{
		int rc = wrc_tuner_quiesce(t);
		if (rc)
			return rc;
	}
	if (keep_state)
		HIP_TRY(hipMemcpy(c.prev_iq, g->dev.prev_iq[g->parity] + 2 * c.slot, 2 * sizeof(float),
		                  hipMemcpyDeviceToHost));
	g->owner[c.slot] = -1;
	g->active--;
	g->dirty = true;
	c.group = -1;
	c.slot = -1;
	c.cs_hist_reset = true;
	c.prev_dirty = keep_state;
	c.phase_dirty = true;
	c.agc_used_on = false;         /* (its envelope stays behind with the slot) */
	return WR_OK;
}

extern "C" int wr_chan_remove(wr_tuner *t, int chan)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_remove: no channel %d", chan);
	int rc = chan_unseat(t, *c, false);
	c->in_use = false;
	return rc;
}

extern "C" int wr_chan_count(wr_tuner *t, int *count)
{
	if (!t || !count)
		return wrc_fail(WR_ERR_ARG, "wr_chan_count: bad argument");
	*count = chans_live(t);
	return WR_OK;
}

/* is this the rate group of a channel with these decimations and filter lengths? */
static bool group_takes(const Group *g, const Chan &c)
{
	return g->d1 == c.decim[0] && g->d2 == c.decim[1] && g->d1b == (c.have[2] ? c.decim[2] : 0u) &&
	       g->l1 == c.len1 && g->l2 == c.len2 && g->l1b == (c.have[2] ? c.len1b : (unsigned int)WR_FIR_LENGTH);
}

/* a setter changed what the channel's group has on the device: uploaded before the next launch */
static void chan_mark_dirty(wr_tuner *t, const Chan *c)
{
	if (c->group >= 0)
		t->groups[c->group]->dirty = true;
}

/* seat a fully configured channel into the group matching its decimations */
static int chan_seat(wr_tuner *t, int idx)
{
	Chan &c = t->chans[idx];
	if (!c.have[0] || !c.have[1])
		return WR_OK;
	if (c.group >= 0) {
		Group *g = t->groups[c.group];
		if (group_takes(g, c)) {
			g->dirty = true;
			return WR_OK;
		}
		int rc = chan_unseat(t, c, true);
		if (rc)
			return rc;
	}
	int gi = -1;
	for (size_t i = 0; i < t->groups.size(); ++i)
		if (group_takes(t->groups[i], c)) {
			gi = (int)i;
			break;
		}
	if (gi < 0) {
		if (wrc_dev_bind(t->dev))
			return WR_ERR_HIP;
		Group *g = nullptr;
		int rc = group_create(t, c.decim[0], c.have[2] ? c.decim[2] : 0u, c.decim[1], c.len1, c.len1b, c.len2, &g);
		if (rc)
			return rc;
		t->groups.push_back(g);
		gi = (int)t->groups.size() - 1;
	}
	Group *g = t->groups[gi];
	int slot = -1;
	for (unsigned int s = 0; s < g->slots; ++s)
		if (g->owner[s] < 0) {
			slot = (int)s;
			break;
		}
	if (slot < 0)
		return wrc_fail(WR_ERR_STATE, "no free slot in rate group %u/%u", g->d1, g->d2);
	g->owner[slot] = idx;
	g->active++;
	g->dirty = true;
	c.group = gi;
	c.slot = slot;
	c.cs_hist_reset = true;        /* fresh LowPass::block: zero history (lowpass.cxx:138-139) */
	c.dem_hist_reset = true;
	c.agc_reset = true;
	c.prev_dirty = true;
	c.phase_dirty = true;
	return WR_OK;
}

extern "C" int wr_chan_set_if(wr_tuner *t, int chan, int if_hz)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_if: no channel %d", chan);
	c->if_hz = if_hz;
	c->stepL = (unsigned int)wrd_phase_step(if_hz, t->input_rate) << 1;
	chan_mark_dirty(t, c);
	return WR_OK;
}

/* `coeff`: 64 taps (a shorter filter zero-extended), or `len` = 128 or 256 of them */
static int set_taps_common(wr_tuner *t, int chan, int stage, const float *coeff, unsigned int decim,
                           unsigned int len = WR_FIR_LENGTH)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "no channel %d", chan);
	if (stage < 0 || stage > 2)
		return wrc_fail(WR_ERR_ARG, "stage must be 0 (channel), 1 (audio) or 2 (second channel filter)");
	if (!decim)
		return wrc_fail(WR_ERR_ARG, "decimation must be >= 1");
	unsigned int *lens[3] = {&c->len1, &c->len2, &c->len1b};
	float *longs[3] = {c->taps_long, c->taps_long2, c->taps_long1b};
	*lens[stage] = len;
	if (len > WR_FIR_LENGTH)
		memcpy(longs[stage], coeff, sizeof(float) * len);
	if (len <= WR_FIR_LENGTH)
		memcpy(c->taps[stage], coeff, sizeof(float) * WR_FIR_LENGTH);
	c->decim[stage] = decim;
	c->have[stage] = true;
	return chan_seat(t, chan);
}

/* LowPass::_firLength as a run-time value in the fused path (lowpass.cxx:38-39 "FIXME: Make runtime
 * variable"): a filter of L <= 64 taps IS the 64-tap filter whose taps L..63 -- the ones that meet
 * the oldest samples -- are zero.  lowpass.cxx:150-158 adds the products oldest sample first, so the
 * padded filter starts with 64 - L products that are +-0 and then runs through exactly the additions
 * of the short one: the same bits (finite input). */
static bool fused_fir_length_ok(unsigned int n)
{
	/* 128 or 256 taps: k_tuner_ddc_long (channel filter), k_tuner_iq2 (second channel stage), k_tuner_demod +
	 * k_tuner_audio (audio filter) with 127 / 255 rows of history -- every stage of the tuner's own launch sequence */
	return n >= 2 && n <= (unsigned int)WR_FIR_FUSED_MAX && (n & (n - 1)) == 0;
}

extern "C" int wr_chan_set_taps_n(wr_tuner *t, int chan, int stage, const float *coeff_host,
                                  unsigned int fir_length, unsigned int decimation)
{
	if (!t || !coeff_host)
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_taps: bad argument");
	if (!fused_fir_length_ok(fir_length))
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_taps_n: fir_length %u is not a power of two in [2, %d] (longer filters run "
		                        "block by block: wr_fir_decimate_n)", fir_length, WR_FIR_FUSED_MAX);
	float coeff[WR_FIR_FUSED_MAX] = {0.0f};
	memcpy(coeff, coeff_host, sizeof(float) * fir_length);
	return set_taps_common(t, chan, stage, coeff, decimation, fir_length > WR_FIR_LENGTH ? fir_length : (unsigned int)WR_FIR_LENGTH);
}

extern "C" int wr_chan_set_taps(wr_tuner *t, int chan, int stage, const float *coeff_host,
                                unsigned int decimation)
{
	return wr_chan_set_taps_n(t, chan, stage, coeff_host, WR_FIR_LENGTH, decimation);
}

extern "C" int wr_chan_set_filter_n(wr_tuner *t, int chan, int stage, unsigned int fir_length,
                                    unsigned int passband, unsigned int out_rate)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_filter: no channel %d", chan);
	if (stage < 0 || stage > 2)
		return wrc_fail(WR_ERR_ARG, "stage must be 0 (channel), 1 (audio) or 2 (second channel filter)");
	if (!fused_fir_length_ok(fir_length))
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_filter_n: fir_length %u is not a power of two in [2, %d]", fir_length,
		                WR_FIR_FUSED_MAX);
	unsigned int in_rate;
	if (stage == 0) {
		in_rate = t->input_rate;
	} else {
		if (!c->have[0])
			return wrc_fail(WR_ERR_STATE, "set the channel filter (stage 0) before the %s", stage == 1 ? "audio filter"
			                : "second channel filter");
		in_rate = t->input_rate / c->decim[0];
		if (stage == 1 && c->have[2])
			in_rate /= c->decim[2];               /* the audio filter follows the LAST channel stage */
	}
	if (!out_rate || out_rate > in_rate)
		return wrc_fail(WR_ERR_RATE, "output rate %u not a decimation of %u", out_rate, in_rate);
	unsigned int decim = in_rate / out_rate;           /* dspblock.cxx:119-121 */
	if (in_rate / decim != out_rate || in_rate % out_rate)
		return wrc_fail(WR_ERR_RATE, "Sample rates must be integer related (%u -> %u)", in_rate, out_rate);
	float coeff[WR_FIR_FUSED_MAX] = {0.0f};
	wrd_lowpass_design(fir_length, passband, in_rate, coeff);
	return set_taps_common(t, chan, stage, coeff, decim, fir_length > WR_FIR_LENGTH ? fir_length : (unsigned int)WR_FIR_LENGTH);
}

extern "C" int wr_chan_set_filter(wr_tuner *t, int chan, int stage, unsigned int passband,
                                  unsigned int out_rate)
{
	return wr_chan_set_filter_n(t, chan, stage, WR_FIR_LENGTH, passband, out_rate);
}

extern "C" int wr_chan_set_mode(wr_tuner *t, int chan, int mode)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_mode: no channel %d", chan);
	if (mode < WR_AM || mode > WR_LSB)
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_mode: bad mode %d", mode);
	c->mode = mode;
	chan_mark_dirty(t, c);
	return WR_OK;
}

/* The two receiver controls the reference's REST interface names and never implements ("FIXME:
 * af_gain, squelch", receiverhandler.cxx:112,127; both reported as 0, :118-119).  Staged like every
 * other setter: they take effect at the next block boundary. */
extern "C" int wr_chan_set_af_gain(wr_tuner *t, int chan, float gain_db)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_af_gain: no channel %d", chan);
	if (!(gain_db == gain_db) || gain_db < -200.0f || gain_db > 200.0f)
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_af_gain: %g dB", (double)gain_db);
	c->gain = (float)pow(10.0, (double)gain_db / 20.0);
	chan_mark_dirty(t, c);
	return WR_OK;
}

extern "C" int wr_chan_set_squelch(wr_tuner *t, int chan, float threshold_dbfs, int enable)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_squelch: no channel %d", chan);
	if (enable && (!(threshold_dbfs == threshold_dbfs) || threshold_dbfs < -300.0f || threshold_dbfs > 100.0f))
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_squelch: %g dBFS", (double)threshold_dbfs);
	c->squelch = enable ? (float)pow(10.0, (double)threshold_dbfs / 10.0) : 0.0f;
	chan_mark_dirty(t, c);
	return WR_OK;
}

/* The control every AM / SSB listener expects beside them: a gain of the receiver's own that follows its audio's
 * level (include/webradio_amd.h: the rule).  Staged like the two above; the kernel's numbers are derived when the group
 * is uploaded, for the audio rate the channel then has. */
extern "C" int wr_chan_set_agc(wr_tuner *t, int chan, float target_dbfs, float decay_db_per_s, float max_gain_db, int enable)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_agc: no channel %d", chan);
	if (enable) {
		float target;
		unsigned int floor_bits, step;
		if (wrd_agc_design(target_dbfs, decay_db_per_s, max_gain_db, 1u, &target, &floor_bits, &step))
			return wrc_fail(WR_ERR_ARG, "wr_chan_set_agc: target %g dBFS (-100 .. 0), decay %g dB/s (0 .. 1e4), largest gain "
			                "%g dB (0 .. 120)", (double)target_dbfs, (double)decay_db_per_s, (double)max_gain_db);
		if (!c->agc_on)
			c->agc_reset = true;                    /* coming on: the envelope starts from floor; new settings keep it */
		c->agc_dbfs = target_dbfs;
		c->agc_decay = decay_db_per_s;
		c->agc_max_gain = max_gain_db;
	}
	c->agc_on = enable != 0;
	chan_mark_dirty(t, c);
	return WR_OK;
}

extern "C" int wr_chan_get_agc(wr_tuner *t, int chan, int *enabled, float *target, unsigned int *floor_bits,
                               unsigned int *step, unsigned int *state)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_get_agc: no channel %d", chan);
	const bool on = c->agc_used_on && c->group >= 0;
	if (enabled)
		*enabled = on ? 1 : 0;
	if (target)
		*target = on ? c->agc_used.target : 0.0f;
	if (floor_bits)
		*floor_bits = on ? c->agc_used.floor_bits : 0u;
	if (step)
		*step = on ? c->agc_used.step : 0u;
	if (state) {
		*state = 0;
		if (on) {
			Group *g = t->groups[c->group];
			if (wrc_dev_bind(t->dev))
				return WR_ERR_HIP;
			if (int rc = wrc_tuner_quiesce(t))
				return rc;
			HIP_TRY(hipMemcpy(state, g->agc_state + c->slot, sizeof(unsigned int), hipMemcpyDeviceToHost));
		}
	}
	return WR_OK;
}

extern "C" int wr_tuner_agc_info(wr_tuner *t, unsigned int *channels_on, unsigned long long *launches)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_agc_info: tuner is NULL");
	if (int rc = wrc_settle_held(t))
		return rc;
	if (channels_on) {
		*channels_on = 0;
		for (const Chan &c : t->chans)
			*channels_on += c.in_use && c.group >= 0 && c.agc_used_on ? 1u : 0u;
	}
	if (launches)
		*launches = t->agc_launches;
	return WR_OK;
}

extern "C" int wr_tuner_keep_stages(wr_tuner *t, unsigned int stage_mask)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (int rc = wrc_settle_held(t))
		return rc;
	t->keep_mask = stage_mask;
	return WR_OK;
}

extern "C" int wr_chan_get_state(wr_tuner *t, int chan, unsigned int *phase, float *prev_iq)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_get_state: no channel %d", chan);
	if (phase)
		*phase = c->phaseL >> 1;
	if (prev_iq) {
		if (c->group >= 0 && !c->prev_dirty) {
			Group *g = t->groups[c->group];
			if (wrc_dev_bind(t->dev))
				return WR_ERR_HIP;
			{
				int rc = wrc_tuner_quiesce(t);
				if (rc)
					return rc;
			}
			HIP_TRY(hipMemcpy(prev_iq, g->dev.prev_iq[g->parity] + 2 * c->slot, 2 * sizeof(float),
			                  hipMemcpyDeviceToHost));
		} else {
			prev_iq[0] = c->prev_iq[0];
			prev_iq[1] = c->prev_iq[1];
		}
	}
	return WR_OK;
}

extern "C" int wr_chan_set_state(wr_tuner *t, int chan, unsigned int phase, const float *prev_iq)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_set_state: no channel %d", chan);
	c->phaseL = phase << 1;
	c->phase_dirty = true;
	if (prev_iq) {
		c->prev_iq[0] = prev_iq[0];
		c->prev_iq[1] = prev_iq[1];
		c->prev_dirty = true;
	}
	chan_mark_dirty(t, c);
	return WR_OK;
}

extern "C" int wr_chan_slot(wr_tuner *t, int chan, int *slot)
{
	Chan *c = chan_get(t, chan);
	if (!c || !slot)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_slot: bad argument");
	if (c->group < 0)
		return wrc_fail(WR_ERR_STATE, "channel %d has no filters yet", chan);
	*slot = c->slot;
	return WR_OK;
}

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
	{
		int rc = wrc_tuner_quiesce(t);
		if (rc)
			return rc;
	}
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
	int rc = prof_drain(t, 0);
	if (rc)
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
				if (int rc = post_send_pending(t, g, false))
					return rc;
			int rc = seek_materialize(t, g);
			if (rc)
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
		if (int rc = post_send_pending(t, g, rode))
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
			int rc = wrc_tuner_launch_held(t);
			if (rc)
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
	{
		int rc = wrc_tuner_launch_held(t);                      /* keep the stream in order */
		if (rc)
			return rc;
	}
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
	int rc = wrc_tuner_launch_held(t);
	if (rc)
		return rc;
	t->coalesce = nblocks;
	return WR_OK;
}

extern "C" int wr_tuner_flush(wr_tuner *t)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	return wrc_tuner_flush(t);
}

extern "C" int wr_chan_fetch(wr_tuner *t, int chan, int stage, float *out_host, size_t out_capacity,
                             size_t *count)
{
	Chan *c = chan_get(t, chan);
	if (!c || !count)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_fetch: bad argument");
	if (c->group < 0 || !t->submitted)
		return wrc_fail(WR_ERR_STATE, "wr_chan_fetch: nothing submitted yet");
	Group *g = t->groups[c->group];
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	{
		int rc = wrc_tuner_flush(t);        /* the block's demod/audio may still be waiting for the next launch */
		if (rc)
			return rc;
	}
	size_t n = 0;
	switch (stage) {
	case WR_STAGE_CHAN_IQ: n = g->last_k1 * 2; break;
	case WR_STAGE_DEMOD:   n = g->last_k1; break;
	case WR_STAGE_AUDIO:   n = g->last_k2; break;
	default: return wrc_fail(WR_ERR_ARG, "wr_chan_fetch: bad stage %d", stage);
	}
	*count = n;
	if (!n)
		return WR_OK;
	if (!out_host || out_capacity < n)
		return wrc_fail(WR_ERR_ARG, "wr_chan_fetch: need room for %zu floats", n);
	const size_t S = g->slots;
	if (stage == WR_STAGE_AUDIO) {
		HIP_TRY(hipMemcpyAsync(out_host, g->dev.audio + (size_t)c->slot * g->k2max, n * sizeof(float),
		                       hipMemcpyDeviceToHost, d->stream));
	} else {
		SCRATCH_GUARD(d);
		int rc = wrc_dev_scratch(d, n);
		if (rc)
			return rc;
		if (stage == WR_STAGE_CHAN_IQ)
			HIP_TRY(wrk_gather_rows(d->stream, t->stream.last_iq ? t->stream.last_iq
			                                   : g->d1b ? g->dev.chan_iq2[g->last_cb] : g->dev.chan_iq[g->last_cb],
			                        g->last_k1, S * 2, (size_t)c->slot * 2, 2, d->scratch));
		else if (!g->last_demod_kept)
			return wrc_fail(WR_ERR_STATE, "wr_chan_fetch: the demodulator output was not kept "
			                "(call wr_tuner_keep_stages(tuner, 1u << WR_STAGE_DEMOD) before submitting)");
		else
			HIP_TRY(wrk_gather_rows(d->stream, g->dev.dem[g->last_parity] + (size_t)(g->l2 - 1) * S, g->last_k1, S,
			                        (size_t)c->slot, 1, d->scratch));
		HIP_TRY(hipMemcpyAsync(out_host, d->scratch, n * sizeof(float), hipMemcpyDeviceToHost, d->stream));
	}
	TUNER_SYNC_CHECKED(t);
	return WR_OK;
}

extern "C" int wr_tuner_audio_dev(wr_tuner *t, const float **audio_dev, size_t *chan_stride,
                                  size_t *frames)
{
	if (!t || !audio_dev || !chan_stride || !frames)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_audio_dev: bad argument");
	if (int rc = wrc_settle_held(t))
		return rc;
	bool several = false;
	Group *g = wrc_single_group(t, &several);
	if (several)
		return wrc_fail(WR_ERR_STATE, "tuner has several rate groups; fetch per channel instead");
	if (!g)
		return wrc_fail(WR_ERR_STATE, "tuner has no configured channel");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	{
		int rc = wrc_tuner_flush(t);        /* the caller is about to read the last block's audio */
		if (rc)
			return rc;
	}
	*audio_dev = g->dev.audio;
	*chan_stride = g->k2max;
	*frames = g->last_k2;
	return WR_OK;
}

/* every receiver's CHANNEL spectrum out of the buffer wr_chan_fetch(WR_STAGE_CHAN_IQ) gathers one column of: the columns
 * are transformed where they lie (k_fft_cols), one launch for the whole group */
extern "C" int wr_tuner_chan_spectra(wr_tuner *t, wr_spectrum *spec, size_t first_frame, float *db_dev, unsigned int *slots)
{
	if (!t || !spec || !db_dev)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_spectra: bad argument (NULL tuner, spectrum or db_dev)");
	if (spec->ch != 2)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_spectra: channel IQ needs an IQ spectrum, this one takes real samples");
	if (spec->n > 8192)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_spectra: fft_size %u is above 8192", spec->n);
	if (spec->dev != t->dev)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_spectra: the spectrum belongs to another device than the tuner");
	if (int rc = wrc_settle_held(t))
		return rc;
	bool several = false;
	Group *g = wrc_single_group(t, &several);
	if (several)
		return wrc_fail(WR_ERR_STATE, "tuner has several rate groups; fetch per channel instead");
	if (!g || !t->submitted)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_chan_spectra: nothing submitted yet");
	if (first_frame > g->last_k1 || spec->n > g->last_k1 - first_frame)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_spectra: frames [%zu, %zu) reach beyond the last submit's %zu channel frames",
		                first_frame, first_frame + spec->n, g->last_k1);
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_flush(t))
		return rc;
	const float *iq = t->stream.last_iq ? t->stream.last_iq : g->d1b ? g->dev.chan_iq2[g->last_cb] : g->dev.chan_iq[g->last_cb];
	/* (the lane groups in use, as wr_tuner_fetch_audio_all counts them; the array's row stride is all of the group's slots) */
	const unsigned int used = wrc_group_slots_used(g);
	if (used)
		HIP_TRY(wrk_fft_cols(d->stream, spec->plan, iq, g->slots, used, first_frame, db_dev, d->num_cus));
	if (slots)
		*slots = used;
	return WR_OK;
}

/* every receiver's signal level out of the same buffer: a pass over it where it lies (k_levels_part, k_levels_sum), the
 * thresholds the group's device arrays hold -- the ones wrc_group_upload gave the last submit */
extern "C" int wr_tuner_chan_levels(wr_tuner *t, float *mean_host, float *peak_host, unsigned int *muted_host, size_t *frames,
                                    size_t *audio_frames, unsigned int *slots)
{
	if (!t || (!mean_host && !peak_host && !muted_host))
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_levels: bad argument (NULL tuner, or no array to fill)");
	if (int rc = wrc_settle_held(t))
		return rc;
	bool several = false;
	Group *g = wrc_single_group(t, &several);
	if (several)
		return wrc_fail(WR_ERR_STATE, "tuner has several rate groups; fetch per channel instead");
	if (!g || !t->submitted)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_chan_levels: nothing submitted yet");
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_flush(t))
		return rc;
	const float *iq = t->stream.last_iq ? t->stream.last_iq : g->d1b ? g->dev.chan_iq2[g->last_cb] : g->dev.chan_iq[g->last_cb];
	const unsigned int used = wrc_group_slots_used(g);
	if (frames)
		*frames = g->last_k1;
	if (audio_frames)
		*audio_frames = g->last_k2;
	if (slots)
		*slots = used;
	if (!used)
		return WR_OK;
	std::vector<float> got((size_t)3 * used, 0.0f);
	if (g->last_k1) {
		SCRATCH_GUARD(d);
		if (int rc = wrc_dev_scratch(d, wrk_chan_levels_work(used, g->last_k1)))
			return rc;
		const float *res = nullptr;
		HIP_TRY(wrk_chan_levels(d->stream, iq, g->slots, used, g->last_k1, g->d2, g->last_k2,
		                        g->use_squelch ? g->dev.squelch : nullptr, d->scratch, &res));
		HIP_TRY(hipMemcpyAsync(got.data(), res, got.size() * sizeof(float), hipMemcpyDeviceToHost, d->stream));
		TUNER_SYNC_CHECKED(t);
	}
	if (mean_host)
		memcpy(mean_host, got.data(), used * sizeof(float));
	if (peak_host)
		memcpy(peak_host, got.data() + used, used * sizeof(float));
	if (muted_host)
		memcpy(muted_host, got.data() + 2u * used, used * sizeof(unsigned int));
	return WR_OK;
}

/* the last submit's audio rows of every channel slot into a tone bank (wr_tones.hip): the rows wr_tuner_audio_dev shows,
 * counted as wr_tuner_chan_levels counts them, read where they lie */
extern "C" int wr_tuner_tones_push(wr_tuner *t, wr_tones *bank, unsigned int *slots)
{
	if (!t || !bank)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_tones_push: bad argument (NULL tuner or bank)");
	if (bank->dev != t->dev)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_tones_push: the bank belongs to another device than the tuner");
	if (int rc = wrc_settle_held(t))
		return rc;
	bool several = false;
	Group *g = wrc_single_group(t, &several);
	if (several)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_tones_push: the tuner has several rate groups");
	if (!g || !t->submitted)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_tones_push: nothing submitted yet");
	const unsigned int used = wrc_group_slots_used(g);
	if (used > bank->max_rows)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_tones_push: the tuner has %u channel slots, the bank %u rows", used, bank->max_rows);
	if (bank->last_tuner == t && bank->last_seq == t->submit_seq)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_tones_push: submit %llu of this tuner is in the bank already", t->submit_seq);
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_flush(t))
		return rc;
	DEV_SETTLE(d);
	if (used && g->last_k2)
		HIP_TRY(wrk_tones_push(d->stream, g->dev.audio, g->k2max, used, g->last_k2, bank->rows, bank->t12, bank->steps,
		                       bank->ntones, bank->window));
	bank->last_tuner = t;
	bank->last_seq = t->submit_seq;
	if (slots)
		*slots = used;
	return WR_OK;
}

extern "C" int wr_tuner_fetch_audio_all(wr_tuner *t, float *out_host, size_t out_capacity,
                                        size_t *chan_stride, size_t *frames, unsigned int *slots_used)
{
	if (!t || !chan_stride || !frames || !slots_used)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_fetch_audio_all: bad argument");
	if (int rc = wrc_settle_held(t))
		return rc;
	bool several = false;
	Group *g = wrc_single_group(t, &several);
	if (several)
		return wrc_fail(WR_ERR_STATE, "tuner has several rate groups; fetch per channel instead");
	if (!g || !t->submitted)
		return wrc_fail(WR_ERR_STATE, "nothing submitted yet");
	unsigned int used = wrc_group_slots_used(g);
	*chan_stride = g->last_k2;
	*frames = g->last_k2;
	*slots_used = used;
	const size_t need = (size_t)used * g->last_k2;
	if (!need)
		return WR_OK;
	if (!out_host || out_capacity < need)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_fetch_audio_all: need room for %zu floats", need);
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	{
		int rc = wrc_tuner_flush(t);
		if (rc)
			return rc;
	}
	HIP_TRY(hipMemcpy2DAsync(out_host, g->last_k2 * sizeof(float), g->dev.audio, g->k2max * sizeof(float),
	                         g->last_k2 * sizeof(float), used, hipMemcpyDeviceToHost, d->stream));
	TUNER_SYNC_CHECKED(t);
	return WR_OK;
}

extern "C" int wr_tuner_submit_count(wr_tuner *t, unsigned long long *submits)
{
	if (!t || !submits)
		return wrc_fail(WR_ERR_ARG, "tuner or submits is NULL");
	*submits = t->submit_seq;                /* (written by submits only: call from the thread that submits) */
	return WR_OK;
}

extern "C" int wr_tuner_set_audio_scale(wr_tuner *t, float scale)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (int rc = wrc_settle_held(t))
		return rc;
	t->audio_scale = scale;
	return WR_OK;
}

extern "C" int wr_chan_reset_history(wr_tuner *t, int chan)
{
	Chan *c = chan_get(t, chan);
	if (!c)
		return g_settle_rc ? g_settle_rc : wrc_fail(WR_ERR_ARG, "wr_chan_reset_history: no channel %d", chan);
	c->cs_hist_reset = true;
	c->dem_hist_reset = true;
	c->agc_reset = true;
	chan_mark_dirty(t, c);
	return WR_OK;
}

/* Time sharding of one stream (BASELINE config 5): every channel of the tuner as if the
 * stream began at `frame` -- both filter histories empty, Demodulator::prev_i/q zero -- except the
 * NCO, whose phase takes the closed-form value it has after `frame` input frames from phase 0
 * (downconverter.cxx:103: phase = frame * phaseStep mod 2^31).  One call for the whole tuner, a
 * handful of stream-ordered fills: no per-channel round trips. */
extern "C" int wr_tuner_seek(wr_tuner *t, unsigned long long frame)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	hipStream_t st = d->stream;
	int rc = wrc_tuner_launch_held(t);
	if (rc)
		return rc;
	for (Group *g : t->groups) {
		if (g->dirty) {
			rc = wrc_group_upload(t, g);
			if (rc)
				return rc;
		}
		/* Lazily where the group's launch can take it (one channel-filter stage of up to 64 taps): nothing is launched
		 * here, the next submit's DDC computes the phase in closed form and reads all-zero state sets, and the post
		 * stage of the chunk before, if it is still waiting, rides in that launch as usual -- a time-sharded stream
		 * (BASELINE config 5) then costs ONE launch per chunk instead of three (seek, DDC, post stage). */
		const bool lazy = !g->d1b && g->l1 <= WR_FIR_LENGTH;
		if (!lazy && g->post_pending)
			/* a post stage still waiting for the next submit would write ITS end-of-block state over ours */
			if ((rc = post_send_pending(t, g, false)) != WR_OK)
				return rc;
		const size_t S = g->slots;
		for (size_t s = 0; s < S; ++s) {
			const int ci = g->owner[s];
			if (ci < 0)
				continue;
			Chan &c = t->chans[ci];
			c.phaseL = (unsigned int)((unsigned long long)c.stepL * frame);     /* host mirror; mod 2^32, left-aligned */
			c.phase_dirty = c.prev_dirty = c.cs_hist_reset = c.dem_hist_reset = false;
			c.prev_iq[0] = c.prev_iq[1] = 0.0f;
			if (c.agc_on) {
				/* the envelope starts from floor again: with the next submit's upload (the one thing a seek leaves staged) */
				c.agc_reset = true;
				g->dirty = true;
			}
		}
		if (lazy) {
			g->seek_pending = true;
			g->seek_frame = frame;
			continue;
		}
		g->seek_pending = false;
		/* on the device from the step array itself: no host data in flight, nothing to wait for */
		HIP_TRY(wrk_seek(st, g->dev, (unsigned int)S, g->sp, g->parity, g->p2, frame));
		if (g->l1 > WR_FIR_LENGTH)
			HIP_TRY(hipMemsetAsync(g->dev.mixhist[g->sp], 0, (size_t)(g->l1 - 1) * S * 2 * sizeof(float), st));
	}
	for (Chan &c : t->chans)
		if (c.in_use && c.group < 0) {
			c.phaseL = (unsigned int)((unsigned long long)c.stepL * frame);
			c.prev_iq[0] = c.prev_iq[1] = 0.0f;
		}
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
