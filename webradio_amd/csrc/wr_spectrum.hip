/*
 * wr_spectrum.hip -- the spectrum sink of the extern "C" boundary declared in include/webradio_amd.h: frames
 * buffered, the newest one transformed (wr_fft.hip), kept aside while a streaming launch is open on the device.
 */
#include "wr_capi_internal.h"

/* --------------------------------------------------------------- spectrum -- */

static int spectrum_create(wr_spectrum **spec, wr_dev *dev, unsigned int fft_size, unsigned int hop, unsigned int ch,
                           const char *who)
{
	if (!spec || !dev)
		return wrc_fail(WR_ERR_ARG, "%s: bad argument", who);
	*spec = nullptr;
	if (fft_size < 8 || fft_size > (1u << 20) || (fft_size & (fft_size - 1)))
		return wrc_fail(WR_ERR_ARG, "size must be a power of 2 in [8, 1048576]");   /* spectrumsink.cxx:53-56 */
	if (hop == 0)
		hop = fft_size;
	if (hop > fft_size)
		return wrc_fail(WR_ERR_ARG, "hop must not exceed fft_size");
	if (wrc_dev_bind(dev))
		return WR_ERR_HIP;
	DEV_SETTLE(dev);
	wr_spectrum *s = new (std::nothrow) wr_spectrum();
	if (!s)
		return wrc_fail(WR_ERR_NOMEM, "out of memory");
	memset(&s->plan, 0, sizeof(s->plan));
	s->dev = dev;
	s->n = fft_size;
	s->hop = hop;
	s->ch = ch;
	s->stage = nullptr;
	s->stage_cap = 0;
	s->pending = 0;
	s->bins = nullptr;
	s->frames_done = 0;

	/* (real samples: the transform that runs is the packed one of fft_size / 2 points, wr_fft.hip) */
	hipError_t e = wrk_fft_plan_create(&s->plan, fft_size, ch);
	if (e == hipSuccess)
		e = hipMalloc((void **)&s->bins, (size_t)fft_size * 2 * sizeof(float));
	if (e != hipSuccess) {
		int rc = wrc_fail(WR_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
		wr_spectrum_destroy(s);
		return rc;
	}
	*spec = s;
	return WR_OK;
}

extern "C" int wr_spectrum_create(wr_spectrum **spec, wr_dev *dev, unsigned int fft_size, unsigned int hop)
{
	return spectrum_create(spec, dev, fft_size, hop, 2, "wr_spectrum_create");
}

/* the reference's FIXMEs at io/spectrumsink.cxx:62-64: one channel, the real-to-complex plan */
extern "C" int wr_spectrum_create_real(wr_spectrum **spec, wr_dev *dev, unsigned int fft_size, unsigned int hop)
{
	return spectrum_create(spec, dev, fft_size, hop, 1, "wr_spectrum_create_real");
}

extern "C" int wr_spectrum_channels(wr_spectrum *s, unsigned int *channels)
{
	if (!s || !channels)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_channels: bad argument");
	*channels = s->ch;
	return WR_OK;
}

extern "C" int wr_spectrum_destroy(wr_spectrum *s)
{
	if (!s)
		return WR_OK;
	(void)hipSetDevice(s->dev->device);
	(void)wrc_dev_stream_sync(s->dev);
	if (s->dev->lazy_stream)
		(void)hipStreamSynchronize(s->dev->lazy_stream);    /* (a deferred frame's copy may be on its way) */
	if (s->def_ev)
		(void)hipEventDestroy(s->def_ev);
	(void)hipHostFree(s->keep_host);
	wrk_fft_plan_free(&s->plan);
	(void)hipFree(s->stage);
	(void)hipFree(s->bins);
	(void)hipFree(s->avg);
	delete s;
	return WR_OK;
}

/* room for `frames` frames in the stage buffer (and a frame more); `carry`: what is pending in the old one moves over */
static int spectrum_stage_room(wr_spectrum *s, size_t frames, bool carry)
{
	if (frames <= s->stage_cap)
		return WR_OK;
	float *nb = nullptr;
	const size_t cap = frames + s->n;
	HIP_TRY(hipMalloc((void **)&nb, cap * s->ch * sizeof(float)));
	if (carry && s->pending)
		HIP_TRY(hipMemcpyAsync(nb, s->stage, s->pending * s->ch * sizeof(float), hipMemcpyDeviceToDevice, s->dev->stream));
	HIP_TRY(wrc_dev_stream_sync(s->dev));                   /* (whatever still reads the old stage) */
	if (s->stage)
		HIP_TRY(hipFree(s->stage));
	s->stage = nb;
	s->stage_cap = cap;
	return WR_OK;
}

/* compact the tail to the front (ranges may overlap: go through the work area): `rest` frames from frame `from` on */
static int spectrum_compact(wr_spectrum *s, size_t from, size_t rest)
{
	wr_dev *d = s->dev;
	hipStream_t st = d->stream;
	const size_t ch = s->ch;
	if (!rest)
		return WR_OK;
	if (rest <= from) {
		HIP_TRY(hipMemcpyAsync(s->stage, s->stage + ch * from, rest * ch * sizeof(float), hipMemcpyDeviceToDevice, st));
	} else {
		SCRATCH_GUARD(d);
		if (int rc = wrc_dev_scratch(d, rest * ch))
			return rc;
		HIP_TRY(hipMemcpyAsync(d->scratch, s->stage + ch * from, rest * ch * sizeof(float), hipMemcpyDeviceToDevice, st));
		HIP_TRY(hipMemcpyAsync(s->stage, d->scratch, rest * ch * sizeof(float), hipMemcpyDeviceToDevice, st));
	}
	return WR_OK;
}

/* a block of `nframes` frames whose newest complete frame starts inside it (wr_spectrum_push: `inside`): the frames it
 * completes, where the newest one starts in THIS block, and the frames behind its hop, which belong to the next frame */
static void spectrum_newest(const wr_spectrum *s, size_t nframes, size_t *nfft, size_t *first, size_t *rest)
{
	const size_t have = s->pending + nframes;
	*nfft = (have - s->n) / s->hop + 1;
	*first = (*nfft - 1) * s->hop - s->pending;
	*rest = have - *nfft * s->hop;
}

/* the deferred frame, if there is one: transformed now, and what follows its hop moved to the stage's front (where the
 * frames carried over to the next push live).  Closes an open streaming launch: once per poll, not once per block. */
static int spectrum_resolve(wr_spectrum *s)
{
	if (!s->deferred)
		return WR_OK;
	wr_dev *d = s->dev;
	DEV_SETTLE(d);
	hipStream_t st = d->stream;
	if (int rc = spectrum_stage_room(s, s->def_keep, false))
		return rc;
	HIP_TRY(hipStreamWaitEvent(st, s->def_ev, 0));
	HIP_TRY(hipMemcpyAsync(s->stage, s->keep_host + 2 * s->def_off, s->def_keep * 2 * sizeof(float), hipMemcpyHostToDevice, st));
	HIP_TRY(wrk_fft_frames(st, s->plan, s->stage, s->hop, 1, s->bins, nullptr));
	const size_t rest = s->def_rest;
	if (int rc = spectrum_compact(s, s->hop, rest))
		return rc;
	s->pending = rest;
	s->deferred = false;
	++s->resolves;
	return WR_OK;
}

/* (r06) a streaming launch is open: keep the frame, transform it when somebody asks (see wr_spectrum::deferred).  A
 * deferred frame of an earlier push that nobody asked for is simply superseded: nobody can observe it any more.
 * `*kept` false: not this way -- the caller goes the ordinary way, which closes the launch. */
static int spectrum_defer(wr_spectrum *s, const float *iq, size_t nframes, bool *kept)
{
	*kept = false;
	wr_dev *d = s->dev;
	size_t nfft, first, rest;
	spectrum_newest(s, nframes, &nfft, &first, &rest);
	const size_t keep = nframes - first;                    /* = n + what follows the frame's hop, of which `rest` belong to the next frame */
	/* WHERE it is kept: in page-locked HOST memory, brought there by the DMA engine.  A device-to-device copy is a copy
	 * KERNEL on this runtime, and a kernel queued beside an open launch is trouble: dispatched while the launch still
	 * fills the chip it holds workgroup slots the launch's own workgroups wait for, and its waves, behind spinning waves
	 * of a higher priority, may never finish -- the launch then runs into its deadline (measured:
	 * 12 of 12 at the device stream's priority, 2 of 8 at the lowest).  Copies of 16 KB or less are kernels too
	 * (GPU_FORCE_BLIT_COPY_SIZE), so at least 4096 frames (32 KB) of the block's end travel. */
	const size_t MINF = 4096;
	const size_t copyf = keep >= MINF ? keep : (nframes >= MINF ? MINF : nframes);
	const size_t off = copyf - keep;
	if (copyf * 2 * sizeof(float) <= 16384u)
		/* (a block of under 2 K frames: nothing the DMA engine would copy -- the ordinary way, which closes the launch) */
		return spectrum_resolve(s);
	if (copyf > s->keep_cap) {
		if (s->keep_host) {
			if (d->lazy_stream)
				HIP_TRY(hipStreamSynchronize(d->lazy_stream));
			(void)hipHostFree(s->keep_host);
			s->keep_host = nullptr;
			s->keep_cap = 0;
		}
		HIP_TRY(hipHostMalloc((void **)&s->keep_host, (copyf + s->n) * 2 * sizeof(float), hipHostMallocDefault));
		s->keep_cap = copyf + s->n;
	}
	{
		std::lock_guard<std::mutex> up_guard(*d->upload_lock);
		if (!d->lazy_stream) {
			int prio_low = 0, prio_high = 0;
			HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
			HIP_TRY(hipStreamCreateWithPriority(&d->lazy_stream, hipStreamNonBlocking, prio_low));
		}
		if (!s->def_ev)
			HIP_TRY(hipEventCreateWithFlags(&s->def_ev, hipEventDisableTiming));
		if (d->up_stream) {
			/* (the block may itself be on its way on the upload stream: behind it) */
			HIP_TRY(hipEventRecord(s->def_ev, d->up_stream));
			HIP_TRY(hipStreamWaitEvent(d->lazy_stream, s->def_ev, 0));
		}
		HIP_TRY(hipMemcpyAsync(s->keep_host, iq + 2 * (first - off), copyf * 2 * sizeof(float), hipMemcpyDeviceToHost, d->lazy_stream));
		HIP_TRY(hipEventRecord(s->def_ev, d->lazy_stream));
	}
	s->def_off = off;
	s->def_keep = keep;
	s->frames_done += nfft;
	s->def_rest = rest;
	s->pending = rest;                                  /* (logically; physically at stage + 2 * hop until resolved) */
	s->deferred = true;
	++s->deferred_pushes;
	*kept = true;
	return WR_OK;
}

extern "C" int wr_spectrum_push(wr_spectrum *s, const float *iq, size_t nframes, int where)
{
	if (!s || (nframes && !iq))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_push: bad argument");
	if (where != WR_HOST && where != WR_DEVICE)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_push: bad `where`");
	wr_dev *d = s->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	const bool inside = where == WR_DEVICE && s->pending + nframes >= s->n &&
	                    ((s->pending + nframes - s->n) / s->hop) * s->hop >= s->pending;   /* the newest frame starts inside this block */
	if (inside && d->streaming && s->ch == 2) {
		/* (IQ only: spectrum_defer's DMA thresholds are sized for tuner blocks; a real spectrum closes the launch) */
		bool kept = false;
		const int rc = spectrum_defer(s, iq, nframes, &kept);
		if (rc || kept)
			return rc;
	}
	if (s->deferred) {
		if (inside) {
			/* this block's newest frame supersedes the deferred one, and reads nothing carried over: drop it */
			s->deferred = false;
		} else if (int rc = spectrum_resolve(s)) {
			return rc;
		}
	}
	DEV_SETTLE(d);
	hipStream_t st = d->stream;
	const size_t ch = s->ch;                                /* floats per frame */
	if (inside) {
		/* A block that already lies in device memory and whose most recent complete frame starts INSIDE it (any block of
		 * fftSize + hop frames or more; whatever was carried over belongs to frames nobody can observe,
		 * spectrumsink.cxx:114-116,136-141): that frame is transformed where it lies and only the tail that belongs to
		 * the NEXT frame is kept -- not the whole block copied into the stage first (32 MB device to device per 4 M-frame
		 * block, and three more enqueues on the host).  Nothing before that frame is read: the caller may have staged the
		 * block's tail only (r04: the host runtime's stagedTail). */
		size_t nfft, first, rest;
		spectrum_newest(s, nframes, &nfft, &first, &rest);
		HIP_TRY(wrk_fft_frames(st, s->plan, iq + ch * first, s->hop, 1, s->bins, nullptr));
		s->frames_done += nfft;
		if (rest) {
			if (int rc = spectrum_stage_room(s, rest, false))
				return rc;
			HIP_TRY(hipMemcpyAsync(s->stage, iq + ch * (first + s->hop), rest * ch * sizeof(float), hipMemcpyDeviceToDevice, st));
		}
		s->pending = rest;
		return WR_OK;
	}
	const size_t have = s->pending + nframes;
	if (int rc = spectrum_stage_room(s, have, true))
		return rc;
	if (nframes)
		HIP_TRY(hipMemcpyAsync(s->stage + ch * s->pending, iq, nframes * ch * sizeof(float),
		                       where == WR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
	/* frames start every `hop`; the reference transforms each one but only the most
	 * recent is observable through getSpectrum (spectrumsink.cxx:114-116,136-141) */
	size_t nfft = 0;
	if (have >= s->n)
		nfft = (have - s->n) / s->hop + 1;
	if (nfft) {
		const float *last = s->stage + ch * (nfft - 1) * s->hop;
		HIP_TRY(wrk_fft_frames(st, s->plan, last, s->hop, 1, s->bins, nullptr));
		s->frames_done += nfft;
		const size_t consumed = nfft * s->hop;
		if (int rc = spectrum_compact(s, consumed, have - consumed))
			return rc;
		s->pending = have - consumed;
	} else {
		s->pending = have;
	}
	if (where == WR_HOST)
		HIP_TRY(wrc_dev_stream_sync(s->dev));
	return WR_OK;
}

extern "C" int wr_spectrum_lazy_info(wr_spectrum *s, unsigned long long *deferred_pushes, unsigned long long *resolves)
{
	if (!s)
		return wrc_fail(WR_ERR_ARG, "spectrum is NULL");
	if (deferred_pushes)
		*deferred_pushes = s->deferred_pushes;
	if (resolves)
		*resolves = s->resolves;
	return WR_OK;
}

extern "C" int wr_spectrum_get_bins(wr_spectrum *s, float *bins_host)
{
	if (!s || !bins_host)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_get_bins: bad argument");
	if (!s->frames_done)
		return wrc_fail(WR_ERR_STATE, "no complete frame yet");
	if (wrc_dev_bind(s->dev))
		return WR_ERR_HIP;
	if (int rc = spectrum_resolve(s))
		return rc;
	HIP_TRY(hipMemcpyAsync(bins_host, s->bins, (size_t)s->n * 2 * sizeof(float), hipMemcpyDeviceToHost,
	                       s->dev->stream));
	HIP_TRY(wrc_dev_stream_sync(s->dev));
	return WR_OK;
}

extern "C" int wr_spectrum_get_db(wr_spectrum *s, float *magnitudes_host)
{
	if (!s || !magnitudes_host)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_get_db: bad argument");
	if (!s->frames_done)
		return wrc_fail(WR_ERR_STATE, "no complete frame yet");
	wr_dev *d = s->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (int rc = spectrum_resolve(s))
		return rc;
	SCRATCH_GUARD(d);
	int rc = wrc_dev_scratch(d, s->n);
	if (rc)
		return rc;
	/* dB + fftshift of the stored bins */
	HIP_TRY(wrk_bins_to_db(d->stream, s->bins, s->n, d->scratch));
	HIP_TRY(hipMemcpyAsync(magnitudes_host, d->scratch, (size_t)s->n * sizeof(float), hipMemcpyDeviceToHost,
	                       d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	return WR_OK;
}

extern "C" int wr_spectrum_get_waterfall_row(wr_spectrum *s, unsigned int width, int hold, float *db_row_host,
                                             uint8_t *palette_host)
{
	if (!s || !width || width > s->n || s->n % width)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_get_waterfall_row: width must divide fft_size");
	if (!s->frames_done)
		return wrc_fail(WR_ERR_STATE, "no complete frame yet");
	wr_dev *d = s->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (int rc = spectrum_resolve(s))
		return rc;
	SCRATCH_GUARD(d);
	int rc = wrc_dev_scratch(d, (size_t)width * 2);
	if (rc)
		return rc;
	float *db_dev = d->scratch;
	uint8_t *pal_dev = (uint8_t *)(d->scratch + width);
	HIP_TRY(wrk_waterfall_row(d->stream, s->bins, s->n, width, hold, db_dev, pal_dev));
	if (db_row_host)
		HIP_TRY(hipMemcpyAsync(db_row_host, db_dev, (size_t)width * sizeof(float), hipMemcpyDeviceToHost, d->stream));
	if (palette_host)
		HIP_TRY(hipMemcpyAsync(palette_host, pal_dev, width, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	return WR_OK;
}

extern "C" int wr_spectrum_frames_done(wr_spectrum *s, unsigned long *frames)
{
	if (!s || !frames)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_frames_done: bad argument");
	*frames = s->frames_done;
	return WR_OK;
}

/* `nframes_fft` frames lying `stride` frames apart to dB rows (wr_spectrum_batch_db: the hop; _rows: the row stride) */
static int spectrum_batch(wr_spectrum *s, const float *iq_dev, size_t stride, size_t nframes_fft, float *db_dev)
{
	if (wrc_dev_bind(s->dev))
		return WR_ERR_HIP;
	DEV_SETTLE(s->dev);
	HIP_TRY(wrk_fft_plan_reserve(&s->plan, nframes_fft, s->dev));   /* (the two-pass transforms' work area: room for the batch) */
	HIP_TRY(wrk_fft_frames(s->dev->stream, s->plan, iq_dev, stride, nframes_fft, nullptr, db_dev));
	return WR_OK;
}

extern "C" int wr_spectrum_batch_db(wr_spectrum *s, const float *iq_dev, size_t nframes_fft, float *db_dev)
{
	if (!s || (nframes_fft && (!iq_dev || !db_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_batch_db: bad argument");
	return spectrum_batch(s, iq_dev, s->hop, nframes_fft, db_dev);
}

extern "C" int wr_spectrum_batch_db_rows(wr_spectrum *s, const float *in_dev, size_t row_stride, size_t nrows, float *db_dev)
{
	if (!s || (nrows && (!in_dev || !db_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_batch_db_rows: bad argument");
	if (row_stride < s->n)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_batch_db_rows: row_stride must not be less than fft_size");
	return spectrum_batch(s, in_dev, row_stride, nrows, db_dev);
}

/* room in the averaging scratch area (grows only; wr_spectrum_destroy frees it) */
static int spectrum_avg_room(wr_spectrum *s, size_t bytes)
{
	if (bytes <= s->avg_bytes)
		return WR_OK;
	HIP_TRY(wrc_dev_stream_sync(s->dev));                   /* (whatever still uses the old area) */
	(void)hipFree(s->avg);
	s->avg = nullptr;
	s->avg_bytes = 0;
	HIP_TRY(hipMalloc((void **)&s->avg, bytes));
	s->avg_bytes = bytes;
	return WR_OK;
}

extern "C" int wr_spectrum_batch_avg(wr_spectrum *s, const float *in_dev, size_t nframes_fft, size_t ngroups, size_t group_stride,
                                     int linear, float *mean_dev, float *peak_dev)
{
	if (!s || !in_dev || (!mean_dev && !peak_dev))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_batch_avg: bad argument");
	if (!nframes_fft)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_batch_avg: nframes_fft must not be 0");
	if (ngroups > 1 && group_stride < s->n)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_batch_avg: group_stride must not be less than fft_size");
	if (!ngroups)
		return WR_OK;
	wr_dev *d = s->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	DEV_SETTLE(d);
	const WrSpecAvgPlan plan = wrp_spec_avg_plan(s->n, nframes_fft, ngroups);
	if (int rc = spectrum_avg_room(s, wrp_spec_avg_bytes(s->n, plan)))
		return rc;
	HIP_TRY(wrk_fft_plan_reserve(&s->plan, plan.fchunk, d));
	float *bins = s->avg, *carry = s->avg + plan.fchunk * plan.gchunk * s->n * 2;
	WrSpecAvgChunk c;
	for (bool more = wrp_spec_avg_next(plan, nframes_fft, ngroups, &c, true); more;
	     more = wrp_spec_avg_next(plan, nframes_fft, ngroups, &c, false)) {
		const float *src = in_dev + s->ch * (c.g0 * group_stride + c.f0 * s->hop);
		HIP_TRY(wrk_fft_groups(d->stream, s->plan, src, s->hop, c.nf, c.ng, group_stride, bins, nullptr));
		HIP_TRY(wrk_spec_reduce(d->stream, bins, s->n, c.ng, c.nf, c.f0 == 0, c.f0 + c.nf == nframes_fft, carry, nframes_fft, linear,
		                        mean_dev ? mean_dev + c.g0 * s->n : nullptr, peak_dev ? peak_dev + c.g0 * s->n : nullptr));
	}
	return WR_OK;
}

extern "C" int wr_spectrum_rows_waterfall(wr_spectrum *s, const float *db_dev, size_t nrows, unsigned int width, int hold,
                                          float *db_rows_dev, uint8_t *palette_dev)
{
	if (!s || (nrows && !db_dev) || (!db_rows_dev && !palette_dev))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_rows_waterfall: bad argument");
	if (!width || width > s->n || s->n % width)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_rows_waterfall: width must divide fft_size");
	if (!nrows)
		return WR_OK;
	wr_dev *d = s->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	DEV_SETTLE(d);
	HIP_TRY(wrk_rows_waterfall(d->stream, db_dev, s->n, nrows, width, hold, db_rows_dev, palette_dev));
	return WR_OK;
}

/* --------------------------------------------------------------- band scan -- */

static bool spectrum_size_ok(unsigned int fft_size)
{
	return fft_size >= 8 && fft_size <= (1u << 20) && !(fft_size & (fft_size - 1));
}

extern "C" int wr_detect_rule_default(unsigned int fft_size, wr_detect_rule *rule)
{
	if (!rule)
		return wrc_fail(WR_ERR_ARG, "wr_detect_rule_default: bad argument");
	if (!spectrum_size_ok(fft_size))
		return wrc_fail(WR_ERR_ARG, "wr_detect_rule_default: fft_size must be a power of 2 in [8, 1048576]");
	rule->bin0 = 0;
	rule->nbins = fft_size;
	rule->span = fft_size < 1024u ? fft_size : 1024u;
	rule->percent = 50;
	rule->threshold = 10.0f;
	rule->linear = 0;
	rule->max_gap = 1;
	rule->min_width = 1;
	return WR_OK;
}

extern "C" int wr_spectrum_bin_hz(unsigned int fft_size, unsigned int sample_rate, double centre_hz, double bin, double *hz)
{
	if (!hz || !sample_rate)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_bin_hz: bad argument");
	if (!spectrum_size_ok(fft_size))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_bin_hz: fft_size must be a power of 2 in [8, 1048576]");
	*hz = centre_hz + (bin - (double)(fft_size / 2u)) * (double)sample_rate / (double)fft_size;
	return WR_OK;
}

extern "C" int wr_spectrum_rows_detect(wr_spectrum *s, const float *rows_dev, size_t nrows, const wr_detect_rule *rule,
                                       unsigned int max_det, wr_detection *det_dev, unsigned int *count_dev, float *floor_dev)
{
	if (!s || !rule || !count_dev || (nrows && !rows_dev) || (max_det && !det_dev))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_rows_detect: bad argument");
	if (const char *field = wrp_detect_rule_bad(s->n, rule))
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_rows_detect: the rule's %s is outside its limits", field);
	if (!nrows)
		return WR_OK;
	wr_dev *d = s->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	DEV_SETTLE(d);
	const WrDetectPlan plan = wrp_detect_plan(rule, nrows);
	if (!floor_dev)
		if (int rc = spectrum_avg_room(s, plan.floor_bytes))
			return rc;
	size_t r0 = 0, nr = 0;
	for (bool more = wrp_detect_next(plan, nrows, &r0, &nr, true); more; more = wrp_detect_next(plan, nrows, &r0, &nr, false))
		HIP_TRY(wrk_detect_rows(d->stream, rows_dev + r0 * s->n, s->n, nr, rule, plan, max_det,
		                        max_det ? det_dev + r0 * max_det : nullptr, count_dev + r0,
		                        floor_dev ? floor_dev + r0 * plan.nspans : s->avg));
	return WR_OK;
}
