/*
 * wr_tuner_read.hip -- what reads the results of a tuner's last submit back: wr_chan_fetch and the whole-tuner readers
 * (audio, channel spectra, signal levels).  All of them see that submit through wrc_last_submit_group and
 * wrc_last_submit_flush, and so do the tone bank and the resampler when they take its audio rows (wr_tuner_tones_push,
 * wr_tuner_resamp_push: wr_banks.hip).  The tuner itself is in wr_tuner.hip, the submit path in wr_tuner_submit.hip.
 */
#include "wr_capi_internal.h"

/* A whole-tuner reader's first step: the held blocks go out, and `v->g` is the tuner's one active rate group.  Refused
 * with WR_ERR_STATE: several groups, or none -- and, with `submitted`, no submit yet.  Nothing is bound or flushed: a
 * reader that refuses a call after this step leaves a pending post stage pending. */
int wrc_last_submit_group(wr_tuner *t, const char *who, bool submitted, WrLastSubmit *v)
{
	if (int rc = wrc_settle_held(t))
		return rc;
	bool several = false;
	v->g = wrc_single_group(t, &several);
	if (several)
		return wrc_fail(WR_ERR_STATE, "%s: the tuner has several rate groups; fetch per channel instead", who);
	if (!v->g && !submitted)
		return wrc_fail(WR_ERR_STATE, "tuner has no configured channel");
	if (!v->g || (submitted && !t->submitted))
		return wrc_fail(WR_ERR_STATE, "%s: nothing submitted yet", who);
	return WR_OK;
}

/* The second step, for the group `v->g`: the device is bound, the last block's post stage has gone out (it may still have
 * been waiting for the next launch), and `v` says where that block's results lie. */
int wrc_last_submit_flush(wr_tuner *t, WrLastSubmit *v)
{
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_flush(t))
		return rc;
	const Group *g = v->g;
	v->used = wrc_group_slots_used(g);
	/* a streaming launch leaves its last block's channel IQ in a buffer of its own; otherwise the demodulator's input is
	 * what the group's last channel stage wrote: the second stage's buffer where there is one */
	v->chan_iq = t->stream.last_iq ? t->stream.last_iq : g->d1b ? g->dev.chan_iq2[g->last_cb] : g->dev.chan_iq[g->last_cb];
	return WR_OK;
}

extern "C" int wr_chan_fetch(wr_tuner *t, int chan, int stage, float *out_host, size_t out_capacity,
                             size_t *count)
{
	Chan *c;
	if (int rc = wrc_chan_get(t, chan, &c, "wr_chan_fetch: bad argument"))
		return rc;
	if (!count)
		return wrc_fail(WR_ERR_ARG, "wr_chan_fetch: bad argument");
	if (c->group < 0 || !t->submitted)
		return wrc_fail(WR_ERR_STATE, "wr_chan_fetch: nothing submitted yet");
	WrLastSubmit v = {t->groups[c->group], 0, nullptr};
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	const Group *g = v.g;
	wr_dev *d = t->dev;
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
		if (int rc = wrc_dev_scratch(d, n))
			return rc;
		if (stage == WR_STAGE_CHAN_IQ)
			HIP_TRY(wrk_gather_rows(d->stream, v.chan_iq, g->last_k1, S * 2, (size_t)c->slot * 2, 2, d->scratch));
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
	WrLastSubmit v;
	if (int rc = wrc_last_submit_group(t, "wr_tuner_audio_dev", false, &v))
		return rc;
	if (int rc = wrc_last_submit_flush(t, &v))          /* the caller is about to read the last block's audio */
		return rc;
	*audio_dev = v.g->dev.audio;
	*chan_stride = v.g->k2max;
	*frames = v.g->last_k2;
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
	WrLastSubmit v;
	if (int rc = wrc_last_submit_group(t, "wr_tuner_chan_spectra", true, &v))
		return rc;
	const Group *g = v.g;
	if (first_frame > g->last_k1 || spec->n > g->last_k1 - first_frame)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_spectra: frames [%zu, %zu) reach beyond the last submit's %zu channel frames",
		                first_frame, first_frame + spec->n, g->last_k1);
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	/* (the lane groups in use, as wr_tuner_fetch_audio_all counts them; the array's row stride is all of the group's slots) */
	if (v.used)
		HIP_TRY(wrk_fft_cols(t->dev->stream, spec->plan, v.chan_iq, g->slots, v.used, first_frame, db_dev, t->dev->num_cus));
	if (slots)
		*slots = v.used;
	return WR_OK;
}

/* every receiver's signal level out of the same buffer: a pass over it where it lies (k_levels_part, k_levels_sum), the
 * thresholds the group's device arrays hold -- the ones wrc_group_upload gave the last submit */
extern "C" int wr_tuner_chan_levels(wr_tuner *t, float *mean_host, float *peak_host, unsigned int *muted_host, size_t *frames,
                                    size_t *audio_frames, unsigned int *slots)
{
	if (!t || (!mean_host && !peak_host && !muted_host))
		return wrc_fail(WR_ERR_ARG, "wr_tuner_chan_levels: bad argument (NULL tuner, or no array to fill)");
	WrLastSubmit v;
	if (int rc = wrc_last_submit_group(t, "wr_tuner_chan_levels", true, &v))
		return rc;
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	const Group *g = v.g;
	wr_dev *d = t->dev;
	const unsigned int used = v.used;
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
		HIP_TRY(wrk_chan_levels(d->stream, v.chan_iq, g->slots, used, g->last_k1, g->d2, g->last_k2,
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

extern "C" int wr_tuner_fetch_audio_all(wr_tuner *t, float *out_host, size_t out_capacity,
                                        size_t *chan_stride, size_t *frames, unsigned int *slots_used)
{
	if (!t || !chan_stride || !frames || !slots_used)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_fetch_audio_all: bad argument");
	WrLastSubmit v;
	if (int rc = wrc_last_submit_group(t, "wr_tuner_fetch_audio_all", true, &v))
		return rc;
	const Group *g = v.g;
	const unsigned int used = wrc_group_slots_used(g);
	*chan_stride = g->last_k2;
	*frames = g->last_k2;
	*slots_used = used;
	const size_t need = (size_t)used * g->last_k2;
	if (!need)
		return WR_OK;
	if (!out_host || out_capacity < need)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_fetch_audio_all: need room for %zu floats", need);
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	HIP_TRY(hipMemcpy2DAsync(out_host, g->last_k2 * sizeof(float), g->dev.audio, g->k2max * sizeof(float),
	                         g->last_k2 * sizeof(float), used, hipMemcpyDeviceToHost, t->dev->stream));
	TUNER_SYNC_CHECKED(t);
	return WR_OK;
}
