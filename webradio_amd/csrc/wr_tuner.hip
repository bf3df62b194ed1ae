/*
 * wr_tuner.hip -- the tuner of the extern "C" boundary declared in include/webradio_amd.h: the object and its rate
 * groups, channels and their staged parameter updates, flush, quiesce, settle and seek.  No DSP arithmetic lives here
 * (design math: wr_design.cpp; kernels: wr_kernels.hip).  Upload and submit are in wr_tuner_submit.hip, what reads a
 * submit's results back in wr_tuner_read.hip, the host half of the streaming launch in wr_tuner_stream.hip, the pinned
 * audio ring in wr_tuner_ring.hip.
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
int wrc_post_send_pending(wr_tuner *t, Group *g, bool rode)
{
	if (!rode)
		HIP_TRY(wrk_tuner_post_args(t->dev->stream, g->post_args));
	g->post_pending = false;
	return wrc_ring_push(t, g, g->pend_seq, g->pend_k2, g->pend_slots, g->pend_direct);
}

/* launch whatever post stage is still pending (results of the last submit wanted now) */
int wrc_tuner_flush(wr_tuner *t)
{
	if (int rc = wrc_tuner_launch_held(t))
		return rc;
	for (Group *g : t->groups) {
		if (!g->post_pending)
			continue;
		if (int rc = wrc_post_send_pending(t, g, false))
			return rc;
	}
	return WR_OK;
}

int wrc_seek_materialize(wr_tuner *t, Group *g)
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
	if (int rc = wrc_tuner_flush(t))
		return rc;
	for (Group *g : t->groups)
		if (int rc = wrc_seek_materialize(t, g))
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

/* what every channel entry point begins with: the held blocks go out (its error, if that fails), then `*c` is channel
 * `chan` -- or WR_ERR_ARG with `what`, the caller's message (a printf format that may name the index with one %d) */
int wrc_chan_get(wr_tuner *t, int chan, Chan **c, const char *what)
{
	if (int rc = wrc_settle_held(t))
		return rc;
	if (!t || chan < 0 || (size_t)chan >= t->chans.size() || !t->chans[chan].in_use)
		return wrc_fail(WR_ERR_ARG, what, chan);
	*c = &t->chans[chan];
	return WR_OK;
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
	if (int rc = wrc_tuner_quiesce(t))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_remove: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_if: no channel %d"))
		return rc;
	c->if_hz = if_hz;
	c->stepL = (unsigned int)wrd_phase_step(if_hz, t->input_rate) << 1;
	chan_mark_dirty(t, c);
	return WR_OK;
}

/* `coeff`: 64 taps (a shorter filter zero-extended), or `len` = 128 or 256 of them */
static int set_taps_common(wr_tuner *t, int chan, int stage, const float *coeff, unsigned int decim,
                           unsigned int len = WR_FIR_LENGTH)
{
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_filter: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_mode: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_af_gain: no channel %d"))
		return rc;
	if (!(gain_db == gain_db) || gain_db < -200.0f || gain_db > 200.0f)
		return wrc_fail(WR_ERR_ARG, "wr_chan_set_af_gain: %g dB", (double)gain_db);
	c->gain = (float)pow(10.0, (double)gain_db / 20.0);
	chan_mark_dirty(t, c);
	return WR_OK;
}

extern "C" int wr_chan_set_squelch(wr_tuner *t, int chan, float threshold_dbfs, int enable)
{
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_squelch: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_agc: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_get_agc: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_get_state: no channel %d"))
		return rc;
	if (phase)
		*phase = c->phaseL >> 1;
	if (prev_iq) {
		if (c->group >= 0 && !c->prev_dirty) {
			Group *g = t->groups[c->group];
			if (wrc_dev_bind(t->dev))
				return WR_ERR_HIP;
			if (int rc = wrc_tuner_quiesce(t))
				return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_set_state: no channel %d"))
		return rc;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_slot: bad argument"))
		return rc;
	if (!slot)
		return wrc_fail(WR_ERR_ARG, "wr_chan_slot: bad argument");
	if (c->group < 0)
		return wrc_fail(WR_ERR_STATE, "channel %d has no filters yet", chan);
	*slot = c->slot;
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
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_reset_history: no channel %d"))
		return rc;
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
	if (int rc = wrc_tuner_launch_held(t))
		return rc;
	for (Group *g : t->groups) {
		if (g->dirty)
			if (int rc = wrc_group_upload(t, g))
				return rc;
		/* Lazily where the group's launch can take it (one channel-filter stage of up to 64 taps): nothing is launched
		 * here, the next submit's DDC computes the phase in closed form and reads all-zero state sets, and the post
		 * stage of the chunk before, if it is still waiting, rides in that launch as usual -- a time-sharded stream
		 * (BASELINE config 5) then costs ONE launch per chunk instead of three (seek, DDC, post stage). */
		const bool lazy = !g->d1b && g->l1 <= WR_FIR_LENGTH;
		if (!lazy && g->post_pending)
			/* a post stage still waiting for the next submit would write ITS end-of-block state over ours */
			if (int rc = wrc_post_send_pending(t, g, false))
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
