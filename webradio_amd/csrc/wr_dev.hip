/*
 * wr_dev.hip -- the device context of the extern "C" boundary declared in include/webradio_amd.h: the error string,
 * the design-helper wrappers, wr_dev_*, the upload streams, and the reference's blocks as one kernel each.  No DSP
 * arithmetic lives here (design math: wr_design.cpp; kernels: wr_kernels.hip, wr_fft.hip).  The tuner is in
 * wr_tuner.hip (submit: wr_tuner_submit.hip, readers: wr_tuner_read.hip, streaming launch: wr_tuner_stream.hip, pinned
 * audio ring: wr_tuner_ring.hip), the spectrum sink in wr_spectrum.hip, the tone bank and the resampler in wr_banks.hip.
 *
 * There is deliberately no CPU code path: every data-path entry point needs a
 * wr_dev, and wr_dev_open fails with WR_ERR_NODEV when HIP reports no device.
 */
#include "wr_capi_internal.h"

/* ------------------------------------------------------------------ errors -- */

static thread_local char g_err[512] = "";

int wrc_fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return code;
}

/* ------------------------------------------------------------------ helpers -- */

/* r05: a streaming launch (wr_tuner_set_streaming) runs until it is told to stop.  Everything that waits for the
 * device's stream, frees device memory (hipFree waits for the device) or must not sit behind an idle launch closes it
 * first; the close is a store to page-locked memory, the launch then finishes the blocks it has and ends. */
int wrc_dev_settle_stream(wr_dev *d)
{
	return d->streaming ? wrc_stream_close(d->streaming) : WR_OK;
}
hipError_t wrc_dev_stream_sync(wr_dev *d)
{
	if (wrc_dev_settle_stream(d))
		return hipErrorUnknown;
	return hipStreamSynchronize(d->stream);
}

int wrc_dev_bind(wr_dev *d)
{
	HIP_TRY(hipSetDevice(d->device));
	return WR_OK;
}

int wrc_dev_scratch(wr_dev *d, size_t floats)
{
	if (d->scratch_floats >= floats)
		return WR_OK;
	if (d->scratch) {
		HIP_TRY(wrc_dev_stream_sync(d));
		HIP_TRY(hipFree(d->scratch));
		d->scratch = nullptr;
		d->scratch_floats = 0;
	}
	HIP_TRY(hipMalloc((void **)&d->scratch, floats * sizeof(float)));
	d->scratch_floats = floats;
	return WR_OK;
}

/* is this host block page-locked?  Its device-side address, or NULL (`why`: what the runtime answered).  Only the
 * probe's OWN error is cleared. */
void *wrc_host_mapped(const void *host, hipError_t *why)
{
	void *mapped = nullptr;
	const hipError_t e = hipHostGetDevicePointer(&mapped, const_cast<void *>(host), 0);
	if (why)
		*why = e;
	if (e != hipSuccess || !mapped) {
		(void)hipGetLastError();
		return nullptr;
	}
	return mapped;
}

/* ------------------------------------------------------------------ misc -- */

extern "C" int wr_abi_version(void) { return WR_ABI_VERSION; }
extern "C" const char *wr_last_error(void) { return g_err; }

extern "C" int wr_tune(int key, long value, long *previous)
{
	if (key != WR_TUNE_DDC_NG2_MIN_PASSES)
		return wrc_fail(WR_ERR_ARG, "wr_tune: unknown key %d", key);
	const long before = wrk_tune_ng2_min_passes(value, true);
	if (previous)
		*previous = before;
	return WR_OK;
}

extern "C" int wr_device_count(int *count)
{
	if (!count)
		return wrc_fail(WR_ERR_ARG, "count is NULL");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) {
		*count = 0;
		return wrc_fail(WR_ERR_NODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
	}
	*count = n;
	return WR_OK;
}

extern "C" int wr_phase_step(int if_hz, unsigned int input_rate, int *phase_step)
{
	if (!phase_step || !input_rate)
		return wrc_fail(WR_ERR_ARG, "wr_phase_step: bad argument");
	*phase_step = wrd_phase_step(if_hz, input_rate);
	return WR_OK;
}

extern "C" int wr_sin_table(float *table_host)
{
	if (!table_host)
		return wrc_fail(WR_ERR_ARG, "table is NULL");
	wrd_sin_table(table_host);
	return WR_OK;
}

extern "C" int wr_lowpass_design(unsigned int passband, unsigned int input_rate, float *coeff_host,
                                 unsigned int *maxbin_out)
{
	if (!coeff_host || !input_rate)
		return wrc_fail(WR_ERR_ARG, "wr_lowpass_design: bad argument");
	wrd_lowpass_design(WR_FIR_LENGTH, passband, input_rate, coeff_host);
	if (maxbin_out)
		*maxbin_out = wrd_lowpass_maxbin(WR_FIR_LENGTH, passband, input_rate);
	return WR_OK;
}

static bool fir_length_ok(unsigned int n)
{
	return n >= 2 && n <= WR_FIR_MAX && (n & (n - 1)) == 0;
}

extern "C" int wr_lowpass_design_n(unsigned int fir_length, unsigned int passband, unsigned int input_rate,
                                   float *coeff_host, unsigned int *maxbin_out)
{
	if (!coeff_host || !input_rate)
		return wrc_fail(WR_ERR_ARG, "wr_lowpass_design_n: bad argument");
	if (!fir_length_ok(fir_length))
		return wrc_fail(WR_ERR_ARG, "wr_lowpass_design_n: fir_length %u is not a power of two in [2, %d]", fir_length,
		                WR_FIR_MAX);
	wrd_lowpass_design(fir_length, passband, input_rate, coeff_host);
	if (maxbin_out)
		*maxbin_out = wrd_lowpass_maxbin(fir_length, passband, input_rate);
	return WR_OK;
}

extern "C" int wr_agc_design(float target_dbfs, float decay_db_per_s, float max_gain_db, unsigned int audio_rate,
                             float *target, unsigned int *floor_bits, unsigned int *step)
{
	if (!target || !floor_bits || !step || !audio_rate)
		return wrc_fail(WR_ERR_ARG, "wr_agc_design: bad argument (a NULL result, or an audio rate of 0)");
	if (wrd_agc_design(target_dbfs, decay_db_per_s, max_gain_db, audio_rate, target, floor_bits, step))
		return wrc_fail(WR_ERR_ARG, "wr_agc_design: target %g dBFS (-100 .. 0), decay %g dB/s (0 .. 1e4), largest gain %g dB "
		                "(0 .. 120), and a floor that is a normal float", (double)target_dbfs, (double)decay_db_per_s,
		                (double)max_gain_db);
	return WR_OK;
}

extern "C" int wr_spectrum_window(unsigned int fft_size, float *window_host)
{
	if (!window_host || !fft_size)
		return wrc_fail(WR_ERR_ARG, "wr_spectrum_window: bad argument");
	wrd_spectrum_window(fft_size, window_host);
	return WR_OK;
}

/* ------------------------------------------------------------------ device -- */

extern "C" int wr_dev_open(wr_dev **dev, int device_index, void *hip_stream)
{
	if (!dev)
		return wrc_fail(WR_ERR_ARG, "dev is NULL");
	*dev = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0)
		return wrc_fail(WR_ERR_NODEV, "no HIP device (%s): this backend has no CPU path",
		                e == hipSuccess ? "count = 0" : hipGetErrorString(e));
	if (device_index < 0 || device_index >= n)
		return wrc_fail(WR_ERR_ARG, "device %d out of range (%d devices)", device_index, n);
	HIP_TRY(hipSetDevice(device_index));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device_index));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return wrc_fail(WR_ERR_NODEV, "device %d is %s; this library is built for gfx950 only",
		                device_index, prop.gcnArchName);

	wr_dev *d = new (std::nothrow) wr_dev();
	if (!d)
		return wrc_fail(WR_ERR_NOMEM, "out of memory");
	/* (value-initialised: every member zero) */
	d->device = device_index;
	d->num_cus = prop.multiProcessorCount;
	/* NULL selects HIP's default (null) stream -- which is also what
	 * torch.cuda.current_stream().cuda_stream is unless the caller switched streams */
	d->stream = (hipStream_t)hip_stream;
	d->own_stream = false;

	std::vector<float> table(WR_TABLE_SIZE), turn(WR_TABLE_SIZE), hi(2 * WR_SPLIT_N), lo(2 * WR_SPLIT_N);
	wrd_sin_table(table.data());
	wrd_sin_table_rounded(turn.data());
	wrd_split_tables(hi.data(), lo.data());
	int rc = WR_OK;
	d->turn_host = (float *)malloc(WR_TABLE_SIZE * sizeof(float));
	d->scratch_lock = new (std::nothrow) std::mutex();
	d->registered = new (std::nothrow) std::map<void *, size_t>();
	d->upload_lock = new (std::nothrow) std::mutex();
	if (!d->turn_host || !d->scratch_lock || !d->registered || !d->upload_lock) {
		free(d->turn_host);
		delete d->scratch_lock;
		delete d->registered;
		delete d->upload_lock;
		delete d;
		return wrc_fail(WR_ERR_NOMEM, "out of memory");
	}
	memcpy(d->turn_host, turn.data(), WR_TABLE_SIZE * sizeof(float));
	do {
		if ((e = hipMalloc((void **)&d->table, WR_TABLE_SIZE * sizeof(float))) != hipSuccess) break;
		if ((e = hipMalloc((void **)&d->table_turn, WR_TABLE_SIZE * sizeof(float))) != hipSuccess) break;
		if ((e = hipMemcpy(d->table_turn, turn.data(), WR_TABLE_SIZE * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
		if ((e = hipMalloc((void **)&d->hi_cs, 2 * WR_SPLIT_N * sizeof(float))) != hipSuccess) break;
		if ((e = hipMalloc((void **)&d->lo_cs, 2 * WR_SPLIT_N * sizeof(float))) != hipSuccess) break;
		if ((e = hipMalloc((void **)&d->coeff, WR_FIR_MAX * sizeof(float))) != hipSuccess) break;
		if ((e = hipMemcpy(d->table, table.data(), WR_TABLE_SIZE * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
		if ((e = hipMemcpy(d->hi_cs, hi.data(), 2 * WR_SPLIT_N * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
		if ((e = hipMemcpy(d->lo_cs, lo.data(), 2 * WR_SPLIT_N * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) break;
	} while (0);
	if (e != hipSuccess) {
		rc = wrc_fail(WR_ERR_HIP, "wr_dev_open: %s", hipGetErrorString(e));
		wr_dev_close(d);
		return rc;
	}
	*dev = d;
	return WR_OK;
}

extern "C" int wr_dev_close(wr_dev *d)
{
	if (!d)
		return WR_OK;
	(void)hipSetDevice(d->device);
	(void)wrc_dev_stream_sync(d);
	(void)hipFree(d->table);
	(void)hipFree(d->table_turn);
	(void)hipFree(d->hi_cs);
	(void)hipFree(d->lo_cs);
	(void)hipFree(d->coeff);
	(void)hipFree(d->scratch);
	free(d->turn_host);
	if (d->registered)
		for (auto &r : *d->registered)              /* what the caller forgot to release */
			(void)hipHostUnregister(r.first);
	delete d->registered;
	delete d->scratch_lock;
	for (int i = 0; i < WR_UPLOAD_RING; ++i)
		if (d->upload_ev[i])
			(void)hipEventDestroy(d->upload_ev[i]);
	delete d->upload_lock;
	if (d->up_stream) {
		(void)hipStreamSynchronize(d->up_stream);
		(void)hipStreamDestroy(d->up_stream);
	}
	for (int i = 0; i < WR_UPLOAD_RING; ++i)
		if (d->up_tail[i])
			(void)hipEventDestroy(d->up_tail[i]);
	if (d->up_done)
		(void)hipEventDestroy(d->up_done);
	(void)hipFree(d->up_raw[0]);
	(void)hipFree(d->up_raw[1]);
	if (d->own_stream)
		(void)hipStreamDestroy(d->stream);
	delete d;
	return WR_OK;
}

extern "C" int wr_dev_sync(wr_dev *d)
{
	if (!d)
		return wrc_fail(WR_ERR_ARG, "dev is NULL");
	wr_tuner *live = d->streaming;                       /* (closed by the sync: its outcome is this call's) */
	HIP_TRY(wrc_dev_stream_sync(d));
	return live ? wrc_stream_check(live) : WR_OK;
}

extern "C" void *wr_dev_stream(wr_dev *d) { return d ? (void *)d->stream : nullptr; }
int wrc_dev_index(const wr_dev *d) { return d->device; }
hipStream_t wrc_dev_stream(const wr_dev *d) { return d->stream; }

extern "C" int wr_dev_malloc(wr_dev *d, size_t bytes, void **ptr_dev)
{
	if (!d || !ptr_dev)
		return wrc_fail(WR_ERR_ARG, "wr_dev_malloc: bad argument");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	HIP_TRY(hipMalloc(ptr_dev, bytes ? bytes : 4));
	HIP_TRY(hipMemsetAsync(*ptr_dev, 0, bytes ? bytes : 4, d->stream));
	return WR_OK;
}

extern "C" int wr_dev_free(wr_dev *d, void *ptr_dev)
{
	if (!d)
		return wrc_fail(WR_ERR_ARG, "dev is NULL");
	if (!ptr_dev)
		return WR_OK;
	HIP_TRY(wrc_dev_stream_sync(d));
	HIP_TRY(hipFree(ptr_dev));
	return WR_OK;
}

extern "C" int wr_dev_upload(wr_dev *d, void *dst_dev, const void *src_host, size_t bytes)
{
	if (!d || (!dst_dev && bytes) || (!src_host && bytes))
		return wrc_fail(WR_ERR_ARG, "wr_dev_upload: bad argument");
	if (!bytes)
		return WR_OK;
	HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	return WR_OK;
}

/* Page-lock a host buffer the caller will upload from repeatedly (a source's block vector): a copy
 * out of pageable memory is staged by the runtime and holds the calling thread for its whole
 * duration; out of registered memory it is one DMA the thread does not wait for. */
extern "C" int wr_dev_host_register(wr_dev *d, void *host, size_t bytes)
{
	if (!d || !host || !bytes)
		return wrc_fail(WR_ERR_ARG, "wr_dev_host_register: bad argument");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	SCRATCH_GUARD(d);
	++d->reg_gen;
	hipError_t e = hipHostRegister(host, bytes, hipHostRegisterDefault);
	if (e == hipErrorHostMemoryAlreadyRegistered) {
		(void)hipGetLastError();
		auto own = d->registered->find(host);
		if (own == d->registered->end())
			/* page-locked by somebody else (the application, torch, another library): that is all
			 * this call is for -- it is neither undone nor recorded, and wr_dev_host_unregister
			 * will leave it alone */
			return WR_OK;
		/* one of OURS whose memory was freed and handed out again by the allocator, perhaps with
		 * another length: register the range as it is now */
		(void)hipHostUnregister(host);
		d->registered->erase(own);
		e = hipHostRegister(host, bytes, hipHostRegisterDefault);
	}
	if (e != hipSuccess) {
		(void)hipGetLastError();                    /* not sticky: a later launch check must not trip over it */
		return wrc_fail(WR_ERR_HIP, "wr_dev_host_register: %s", hipGetErrorString(e));
	}
	(*d->registered)[host] = bytes;
	return WR_OK;
}

extern "C" int wr_dev_host_unregister(wr_dev *d, void *host)
{
	if (!d || !host)
		return wrc_fail(WR_ERR_ARG, "wr_dev_host_unregister: bad argument");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	SCRATCH_GUARD(d);
	auto own = d->registered->find(host);
	if (own == d->registered->end())
		return WR_OK;                               /* not page-locked by this library: not ours to release */
	d->registered->erase(own);
	++d->reg_gen;
	hipError_t e = hipHostUnregister(host);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return wrc_fail(WR_ERR_HIP, "wr_dev_host_unregister: %s", hipGetErrorString(e));
	}
	return WR_OK;
}

/* Enqueue a host-to-device copy on the device's stream and return; the host buffer must stay
 * untouched until wr_dev_wait_uploads (or wr_dev_sync) returns. */
/* marks "the upload just enqueued on the stream ends here"; the event it reuses belonged to the upload WR_UPLOAD_RING
 * before it, which is waited for first if nobody has yet */
int wrc_upload_mark_locked(wr_dev *d, hipStream_t st)
{
	const unsigned long long n = d->uploads_issued + 1;
	hipEvent_t &ev = d->upload_ev[n % WR_UPLOAD_RING];
	if (!ev)
		HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	else if (n > WR_UPLOAD_RING && d->uploads_done < n - WR_UPLOAD_RING) {
		HIP_TRY(hipEventSynchronize(ev));
		d->uploads_done = n - WR_UPLOAD_RING;
	}
	HIP_TRY(hipEventRecord(ev, st));
	d->uploads_issued = n;
	return WR_OK;
}

int wrc_upload_mark(wr_dev *d, hipStream_t st)
{
	std::lock_guard<std::mutex> g(*d->upload_lock);
	return wrc_upload_mark_locked(d, st);
}

extern "C" int wr_dev_upload_async(wr_dev *d, void *dst_dev, const void *src_host, size_t bytes)
{
	if (!d || (bytes && (!dst_dev || !src_host)))
		return wrc_fail(WR_ERR_ARG, "wr_dev_upload_async: bad argument");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (bytes)
		HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, d->stream));
	return wrc_upload_mark(d, d->stream);
}

extern "C" int wr_dev_wait_uploads_but(wr_dev *d, unsigned int newest)
{
	if (!d)
		return wrc_fail(WR_ERR_ARG, "dev is NULL");
	if (newest >= WR_UPLOAD_RING)
		return wrc_fail(WR_ERR_ARG, "wr_dev_wait_uploads_but: at most %d uploads can be left in flight", WR_UPLOAD_RING - 1);
	if (d->uploads_issued <= d->uploads_done + newest)
		return WR_OK;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	std::lock_guard<std::mutex> g(*d->upload_lock);
	const unsigned long long issued = d->uploads_issued;
	if (issued <= d->uploads_done + newest)
		return WR_OK;
	/* uploads 1..upto must have completed.  They are not all on one stream (wr_dev_upload_async: the device's;
	 * wr_dev_upload_ahead / wr_u8_to_f32_from_host: the upload stream), so the event of upload `upto` does not speak
	 * for the ones before it: every event in (done, upto] is waited for -- at most WR_UPLOAD_RING - 1 of them, the
	 * issuing side never lets more stay open */
	const unsigned long long upto = issued - newest;
	for (unsigned long long i = d->uploads_done + 1; i <= upto; ++i)
		HIP_TRY(hipEventSynchronize(d->upload_ev[i % WR_UPLOAD_RING]));
	d->uploads_done = upto;
	return WR_OK;
}

extern "C" int wr_dev_wait_uploads(wr_dev *d)
{
	return wr_dev_wait_uploads_but(d, 0);
}

extern "C" int wr_dev_download(wr_dev *d, void *dst_host, const void *src_dev, size_t bytes)
{
	if (!d || (!dst_host && bytes) || (!src_dev && bytes))
		return wrc_fail(WR_ERR_ARG, "wr_dev_download: bad argument");
	if (!bytes)
		return WR_OK;
	wr_tuner *live = d->streaming;
	HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	return live ? wrc_stream_check(live) : WR_OK;
}

/* --------------------------------------------------- one kernel per block -- */

/* how often this process has run one of the reference's blocks as a stand-alone kernel (wr_mix, wr_fir_decimate(_n),
 * wr_demod): what a Receiver that is NOT in a tuner batch costs per block -- a test that expects a chain to stay in the
 * batch reads 0 here */
static std::atomic<unsigned long long> g_block_kernel_calls{0};
extern "C" unsigned long long wr_block_kernel_calls(void)
{
	return g_block_kernel_calls.load(std::memory_order_relaxed);
}
void wrc_block_kernel_called(void)                       /* (the plain-rows pushes of wr_banks.hip count here too) */
{
	g_block_kernel_calls.fetch_add(1, std::memory_order_relaxed);
}

extern "C" int wr_mix(wr_dev *d, const float *in_dev, float *out_dev, size_t nframes,
                      unsigned int *phase_io, int phase_step)
{
	if (!d || !phase_io || (nframes && (!in_dev || !out_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_mix: bad argument");
	DEV_SETTLE(d);
	g_block_kernel_calls.fetch_add(1, std::memory_order_relaxed);
	HIP_TRY(wrk_mix(d->stream, in_dev, out_dev, nframes, *phase_io, phase_step, d->table));
	/* DownConverter::phase after nframes increments (downconverter.cxx:103) */
	*phase_io = (*phase_io + (unsigned int)nframes * (unsigned int)phase_step) & 0x7FFFFFFFu;
	return WR_OK;
}

extern "C" int wr_fir_decimate_n(wr_dev *d, const float *in_dev, size_t nframes, unsigned int channels,
                                 unsigned int decimation, unsigned int fir_length, const float *coeff_host,
                                 float *history_dev, float *out_dev)
{
	if (!d || !coeff_host || !history_dev || !channels || !decimation ||
	    (nframes && (!in_dev || !out_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_fir_decimate: bad argument");
	if (!fir_length_ok(fir_length))
		return wrc_fail(WR_ERR_ARG, "wr_fir_decimate: fir_length %u is not a power of two in [2, %d]", fir_length,
		                WR_FIR_MAX);
	DEV_SETTLE(d);
	SCRATCH_GUARD(d);
	int rc = wrc_dev_scratch(d, (size_t)(fir_length - 1) * channels);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpyAsync(d->coeff, coeff_host, fir_length * sizeof(float), hipMemcpyHostToDevice, d->stream));
	g_block_kernel_calls.fetch_add(1, std::memory_order_relaxed);
	HIP_TRY(wrk_fir(d->stream, in_dev, nframes, channels, decimation, fir_length, d->coeff, history_dev, out_dev));
	HIP_TRY(wrk_hist_update(d->stream, in_dev, nframes, channels, fir_length, history_dev, d->scratch));
	return WR_OK;
}

extern "C" int wr_fir_decimate(wr_dev *d, const float *in_dev, size_t nframes, unsigned int channels,
                               unsigned int decimation, const float *coeff_host, float *history_dev,
                               float *out_dev)
{
	return wr_fir_decimate_n(d, in_dev, nframes, channels, decimation, WR_FIR_LENGTH, coeff_host, history_dev,
	                         out_dev);
}

extern "C" int wr_demod(wr_dev *d, int mode, const float *in_dev, size_t nframes, float *prev_io,
                        float *out_dev)
{
	if (!d || !prev_io || (nframes && (!in_dev || !out_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_demod: bad argument");
	if (mode < WR_AM || mode > WR_LSB)
		return wrc_fail(WR_ERR_ARG, "wr_demod: bad mode %d", mode);   /* demodulator.cxx:105-107 */
	g_block_kernel_calls.fetch_add(1, std::memory_order_relaxed);
	DEV_SETTLE(d);
	HIP_TRY(wrk_demod(d->stream, mode, in_dev, nframes, prev_io[0], prev_io[1], out_dev));
	if (nframes) {
		/* prev_i/q = last input frame (demodulator.cxx:110-111) */
		HIP_TRY(hipMemcpyAsync(prev_io, in_dev + 2 * (nframes - 1), 2 * sizeof(float),
		                       hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(wrc_dev_stream_sync(d));
	}
	return WR_OK;
}

/* the level of a plain block: wr_tuner_chan_levels' kernels on ONE column (S = 1, cols = 1) */
extern "C" int wr_iq_levels(wr_dev *d, const float *iq_dev, size_t nframes, float *mean_host, float *peak_host)
{
	if (!d || !iq_dev || !nframes)
		return wrc_fail(WR_ERR_ARG, "wr_iq_levels: bad argument (NULL dev or iq_dev, or no frames)");
	g_block_kernel_calls.fetch_add(1, std::memory_order_relaxed);
	DEV_SETTLE(d);
	float got[3];
	{
		SCRATCH_GUARD(d);
		if (int rc = wrc_dev_scratch(d, wrk_chan_levels_work(1, nframes)))
			return rc;
		const float *res = nullptr;
		HIP_TRY(wrk_chan_levels(d->stream, iq_dev, 1, 1, nframes, 0, 0, nullptr, d->scratch, &res));
		HIP_TRY(hipMemcpyAsync(got, res, sizeof(got), hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(wrc_dev_stream_sync(d));
	}
	if (mean_host)
		*mean_host = got[0];
	if (peak_host)
		*peak_host = got[1];
	return WR_OK;
}

/* the AGC of a plain audio block (or of several rows of one): the tuner's kernel, parameters and state through scratch */
extern "C" int wr_agc_rows(wr_dev *d, float *audio_dev, size_t row_stride, size_t nrows, size_t nframes,
                           const float *target_host, const unsigned int *floor_bits_host, const unsigned int *step_host,
                           unsigned int *state_host)
{
	if (!d || !audio_dev || !target_host || !floor_bits_host || !step_host || !state_host || !nrows || nrows > 0x7fffffffu ||
	    (nrows > 1 && row_stride < nframes))
		return wrc_fail(WR_ERR_ARG, "wr_agc_rows: bad argument (a NULL pointer, no rows, or rows that overlap)");
	std::vector<WrAgcPar> par(nrows);
	for (size_t r = 0; r < nrows; ++r) {
		par[r] = WrAgcPar{target_host[r], floor_bits_host[r], step_host[r], 1.0f};
		if (step_host[r] == WR_AGC_OFF)
			continue;
		/* the envelope stays a positive, finite, normal float: floor is one, and the state is none above FLT_MAX */
		if (step_host[r] > 0x80000000u || floor_bits_host[r] < 0x00800000u || floor_bits_host[r] > 0x7f7fffffu ||
		    state_host[r] > 0x7f7fffffu || !(target_host[r] > 0.0f) || !(target_host[r] <= 3.40282347e+38f))
			return wrc_fail(WR_ERR_ARG, "wr_agc_rows: row %zu: step %u, floor bits 0x%08x, state 0x%08x, target %g", r,
			                step_host[r], floor_bits_host[r], state_host[r], (double)target_host[r]);
	}
	if (!nframes)
		return WR_OK;
	g_block_kernel_calls.fetch_add(1, std::memory_order_relaxed);
	DEV_SETTLE(d);
	SCRATCH_GUARD(d);
	if (int rc = wrc_dev_scratch(d, nrows * 5u))
		return rc;
	WrAgcPar *par_dev = (WrAgcPar *)d->scratch;
	unsigned int *state_dev = (unsigned int *)(d->scratch + nrows * 4u);
	HIP_TRY(hipMemcpyAsync(par_dev, par.data(), nrows * sizeof(WrAgcPar), hipMemcpyHostToDevice, d->stream));
	HIP_TRY(hipMemcpyAsync(state_dev, state_host, nrows * sizeof(unsigned int), hipMemcpyHostToDevice, d->stream));
	HIP_TRY(wrk_agc_rows(d->stream, audio_dev, row_stride, nrows, nframes, par_dev, state_dev, 1.0f));
	HIP_TRY(hipMemcpyAsync(state_host, state_dev, nrows * sizeof(unsigned int), hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	return WR_OK;
}

extern "C" int wr_u8_to_f32(wr_dev *d, const uint8_t *in_dev, float *out_dev, size_t count)
{
	if (!d || (count && (!in_dev || !out_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_u8_to_f32: bad argument");
	DEV_SETTLE(d);
	HIP_TRY(wrk_u8_to_f32(d->stream, in_dev, out_dev, count));
	return WR_OK;
}

/* The upload stream (wr_dev_upload_ahead, wr_u8_to_f32_from_host): a block crosses PCIe beside whatever the device's stream
 * is doing with the block before (8 MB take 150 us at 55 GB/s -- more than all the kernels of a C2 block together).
 * upload_ahead_begin makes the upload stream wait for the last readers of `out_dev`: those were enqueued before the call
 * that followed the last one to write `out_dev` (a caller alternating between two buffers: before the previous call), or --
 * the same buffer twice in a row, or one not seen lately -- by now.  upload_ahead_end makes the device's stream wait for
 * what was put on the upload stream in between and marks the upload (wr_dev_wait_uploads).  Under d->upload_lock. */
int wrc_dev_up_stream(wr_dev *d)
{
	if (!d->up_stream) {
		int prio_low = 0, prio_high = 0;                     /* lowest priority: the kernels of the block before go first */
		HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
		HIP_TRY(hipStreamCreateWithPriority(&d->up_stream, hipStreamNonBlocking, prio_low));
		/* up_done (recorded on the upload stream: nothing of the device's stream pays for it) publishes the copied block and keeps
		 * the default fence; up_tail only keeps the copy from overwriting what earlier work still reads: a device-scope release */
		HIP_TRY(hipEventCreateWithFlags(&d->up_done, hipEventDisableTiming));
		for (int i = 0; i < WR_UPLOAD_RING; ++i)
			HIP_TRY(hipEventCreateWithFlags(&d->up_tail[i], hipEventDisableTiming | hipEventReleaseToDevice));
	}
	return WR_OK;
}

static int upload_ahead_begin(wr_dev *d, void *out_dev, unsigned long long *call)
{
	if (int rc = wrc_dev_up_stream(d))
		return rc;
	const unsigned long long n = d->up_calls;
	HIP_TRY(hipEventRecord(d->up_tail[n % WR_UPLOAD_RING], d->stream));
	unsigned long long after = n;                      /* wait for the tail recorded by call `after` */
	for (unsigned long long back = 1; back < WR_UPLOAD_RING && back <= n; ++back)
		if (d->up_out[(n - back) % WR_UPLOAD_RING] == out_dev) {
			after = n - back + 1;
			break;
		}
	HIP_TRY(hipStreamWaitEvent(d->up_stream, d->up_tail[after % WR_UPLOAD_RING], 0));
	d->up_out[n % WR_UPLOAD_RING] = out_dev;
	d->up_calls = n + 1;
	*call = n;
	return WR_OK;
}

static int upload_ahead_end(wr_dev *d)
{
	HIP_TRY(hipEventRecord(d->up_done, d->up_stream));
	HIP_TRY(hipStreamWaitEvent(d->stream, d->up_done, 0));
	return wrc_upload_mark_locked(d, d->up_stream);
}

extern "C" int wr_dev_upload_ahead(wr_dev *d, void *dst_dev, const void *src_host, size_t bytes)
{
	if (!d || (bytes && (!dst_dev || !src_host)))
		return wrc_fail(WR_ERR_ARG, "wr_dev_upload_ahead: bad argument");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	std::lock_guard<std::mutex> up_guard(*d->upload_lock);
	unsigned long long n = 0;
	if (int rc = upload_ahead_begin(d, dst_dev, &n))
		return rc;
	if (bytes)
		HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, d->up_stream));
	return upload_ahead_end(d);
}

extern "C" int wr_u8_to_f32_from_host(wr_dev *d, const uint8_t *in_host, float *out_dev, size_t count)
{
	if (!d || (count && (!in_host || !out_dev)))
		return wrc_fail(WR_ERR_ARG, "wr_u8_to_f32_from_host: bad argument");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	hipError_t e = hipSuccess;
	if (!wrc_host_mapped(in_host, &e))
		return wrc_fail(WR_ERR_ARG, "wr_u8_to_f32_from_host: the buffer is not page-locked (wr_dev_host_register): %s",
		                hipGetErrorString(e));
	std::lock_guard<std::mutex> up_guard(*d->upload_lock);         /* the ring of tails: calls may come from several threads */
	/* The bytes come over with the DMA engine and are converted out of device memory.  (r03 tried the kernel reading
	 * host memory itself: one launch and 47 GB/s -- but kernels running beside it take up to ten times
	 * as long, k_tuner_post 14 -> 107 us, a 32 MB device copy 13 -> 146 us: its reads, microseconds each, sit in the
	 * same L2 / fabric queues as everybody's HBM traffic.  A DMA copy does not go through them.) */
	/* Only the COPY runs on the upload stream, into one of two raw buffers in turn; the conversion follows on the device's
	 * stream once the copy's event has fired.  So the copies of consecutive blocks follow each other on the link without
	 * a kernel in between (the upload stream waits for nothing but the conversion that last read the raw buffer it is about
	 * to overwrite -- two calls ago), and `out_dev` is written in stream order like any kernel's output. */
	const unsigned int rb = (unsigned int)(d->up_calls & 1u);
	if (d->up_raw_cap[rb] < count) {
		if (d->up_stream)
			HIP_TRY(hipStreamSynchronize(d->up_stream));
		HIP_TRY(wrc_dev_stream_sync(d));
		(void)hipFree(d->up_raw[rb]);
		d->up_raw[rb] = nullptr;
		d->up_raw_cap[rb] = 0;
		HIP_TRY(hipMalloc((void **)&d->up_raw[rb], count));
		d->up_raw_cap[rb] = count;
	}
	unsigned long long n = 0;
	if (int rc = upload_ahead_begin(d, (void *)d->up_raw[rb], &n))
		return rc;
	HIP_TRY(hipMemcpyAsync(d->up_raw[rb], in_host, count, hipMemcpyHostToDevice, d->up_stream));
	if (int rc = upload_ahead_end(d))                          /* the host buffer is free again when the COPY is done */
		return rc;
	HIP_TRY(wrk_u8_to_f32(d->stream, d->up_raw[rb], out_dev, count));
	return WR_OK;
}

extern "C" int wr_stage_windows_from_host(wr_dev *d, const void *in_host, int is_u8, float *out_dev, size_t nframes,
                                          unsigned int period, unsigned int length, size_t tail_frames)
{
	if (!d || (nframes && (!in_host || !out_dev)) || !period || !length)
		return wrc_fail(WR_ERR_ARG, "wr_stage_windows_from_host: bad argument");
	if (length > 4096u)
		return wrc_fail(WR_ERR_ARG, "wr_stage_windows_from_host: windows of %u frames", length);
	if (((uintptr_t)in_host | (uintptr_t)out_dev) & 15u)
		return wrc_fail(WR_ERR_ARG, "wr_stage_windows_from_host: both buffers must be 16-byte aligned");
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	hipError_t e = hipSuccess;
	void *mapped = wrc_host_mapped(in_host, &e);
	if (!mapped)
		return wrc_fail(WR_ERR_ARG, "wr_stage_windows_from_host: the buffer is not page-locked (wr_dev_host_register): %s",
		                hipGetErrorString(e));
	HIP_TRY(wrk_stage_windows(d->stream, mapped, is_u8 != 0, out_dev, nframes, period, length, tail_frames));
	return wrc_upload_mark(d, d->stream);                  /* the host buffer is free again when the kernel has read it */
}
