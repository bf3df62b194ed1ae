/*
 * wr_banks.hip -- the four objects that keep something per audio row of every receiver: the tone bank (wr_tones_*, kernels
 * in wr_tones.hip), the DCS bank (wr_dcs_*, kernel in wr_dcs.hip), the resampler (wr_resamp_*, kernels in wr_resamp.hip) and
 * the voice bank (wr_voice_*, kernel in wr_voice.hip).
 * Each takes plain rows (wr_*_push_rows) or the audio rows of a tuner's last submit where they lie (wr_tuner_*_push); what
 * the four share has one copy, up front.
 */
#include "wr_capi_internal.h"

/* ------------------------------------------------------------------ shared (`who`: the entry point a message names) -- */

/* the device bound and no streaming launch open on its stream; `block_call`: counted by wr_block_kernel_calls() */
static int bank_dev_ready(wr_dev *d, bool block_call)
{
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (block_call)
		wrc_block_kernel_called();
	return wrc_dev_settle_stream(d);
}

/* a create, before its device memory: a T of `max_rows` rows (value-initialised: every other member zero) on a device made ready */
template <class T> static int bank_new(T **b, const char *who, wr_dev *d, unsigned int max_rows)
{
	if (int rc = bank_dev_ready(d, false))
		return rc;
	if (!(*b = new (std::nothrow) T()))
		return wrc_fail(WR_ERR_ARG, "%s: out of memory", who);
	(*b)->dev = d;
	(*b)->max_rows = max_rows;
	return WR_OK;
}

/* ... and behind it: the uploads have been waited for (their sources are the call's or the caller's), or the bank goes again */
template <class T> static int bank_created(T **out, T *b, hipError_t e, const char *who, int (*destroy)(T *))
{
	if (e == hipSuccess)
		e = wrc_dev_stream_sync(b->dev);
	if (e != hipSuccess) {
		destroy(b);
		return wrc_fail(WR_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
	}
	*out = b;
	return WR_OK;
}

/* what a push of plain rows refuses: more rows than the bank has, rows that overlap, more than 2^max_log2 frames */
static int bank_rows_refused(const WrRowBank *b, const char *who, size_t row_stride, size_t nrows, size_t nframes,
                             unsigned int max_log2)
{
	if (nrows > b->max_rows || (nrows > 1 && row_stride < nframes) || nframes > ((size_t)1 << max_log2))
		return wrc_fail(WR_ERR_ARG, "%s: %zu rows for a bank of %u, or rows of %zu frames that overlap at a stride of %zu, or more "
		                "than 2^%u frames", who, nrows, b->max_rows, nframes, row_stride, max_log2);
	return WR_OK;
}

/* a reset's first steps: `row` is one of the bank's, or negative for all of them -- `n` rows from `first` -- and the device is ready */
static int bank_reset_begin(const WrRowBank *b, const char *who, int row, size_t *first, size_t *n)
{
	if (row >= 0 && (unsigned int)row >= b->max_rows)
		return wrc_fail(WR_ERR_ARG, "%s: row %d of a bank of %u", who, row, b->max_rows);
	*first = row < 0 ? 0 : (size_t)row;
	*n = row < 0 ? b->max_rows : 1;
	return bank_dev_ready(b->dev, false);
}

/* A tuner push's first step: `v->g` is the tuner's one rate group, `v->used` its slots in use -- the rows of the push.  Refused
 * (`noun`: what a message calls the object): a bank of another device, what wrc_last_submit_group refuses, more slots than
 * rows, and the submit the bank took last.  Nothing is bound or flushed.  (A tuner is known by its address: a destroyed one's
 * successor at the same address and submit count is refused once.) */
static int bank_take_submit(const WrRowBank *b, const char *who, const char *noun, wr_tuner *t, WrLastSubmit *v)
{
	if (b->dev != t->dev)
		return wrc_fail(WR_ERR_ARG, "%s: the %s belongs to another device than the tuner", who, noun);
	if (int rc = wrc_last_submit_group(t, who, true, v))
		return rc;
	v->used = wrc_group_slots_used(v->g);
	if (v->used > b->max_rows)
		return wrc_fail(WR_ERR_ARG, "%s: the tuner has %u channel slots, the %s %u rows", who, v->used, noun, b->max_rows);
	if (b->last_tuner == t && b->last_seq == t->submit_seq)
		return wrc_fail(WR_ERR_STATE, "%s: submit %llu of this tuner is in the %s already", who, t->submit_seq, noun);
	return WR_OK;
}

/* ... and its last, once the push has gone out */
static int bank_took_submit(WrRowBank *b, const wr_tuner *t, const WrLastSubmit &v, unsigned int *slots)
{
	b->last_tuner = t;
	b->last_seq = t->submit_seq;
	if (slots)
		*slots = v.used;
	return WR_OK;
}

/* ------------------------------------------------------------------ tone bank -- */

extern "C" int wr_tone_step(double hz, unsigned int audio_rate, unsigned int *step)
{
	if (!step)
		return wrc_fail(WR_ERR_ARG, "wr_tone_step: step is NULL");
	if (wrd_tone_step(hz, audio_rate, step))
		return wrc_fail(WR_ERR_ARG, "wr_tone_step: %g Hz is not inside (0, %g), half the audio rate", hz, (double)audio_rate / 2.0);
	return WR_OK;
}

extern "C" int wr_tones_create(wr_tones **bank, wr_dev *d, unsigned int max_rows, const unsigned int *steps_host,
                               unsigned int ntones, unsigned int window)
{
	if (!bank || !d || !steps_host)
		return wrc_fail(WR_ERR_ARG, "wr_tones_create: bad argument (NULL bank, dev or steps_host)");
	if (!max_rows || max_rows > 65535u || !ntones || ntones > WR_LANES || window < 16u || window > 65536u)
		return wrc_fail(WR_ERR_ARG, "wr_tones_create: %u rows (1 .. 65535), %u tones (1 .. 64), a window of %u frames "
		                "(16 .. 65536)", max_rows, ntones, window);
	unsigned int steps[WR_LANES] = {0};
	for (unsigned int t = 0; t < ntones; ++t) {
		if (!steps_host[t] || steps_host[t] >= 0x80000000u)
			return wrc_fail(WR_ERR_ARG, "wr_tones_create: tone %u: a step of %u is not inside (0, 2^31)", t, steps_host[t]);
		steps[t] = steps_host[t];
	}
	std::vector<float> table(WR_TABLE_SIZE), t12(4096);
	wrd_sin_table(table.data());
	for (unsigned int i = 0; i < 4096u; ++i)
		t12[i] = table[16u * i];
	wr_tones *b;
	if (int rc = bank_new(&b, "wr_tones_create", d, max_rows))
		return rc;
	b->ntones = ntones;
	b->window = window;
	hipError_t e = hipMalloc((void **)&b->rows, (size_t)max_rows * sizeof(WrTonesRow));
	if (e == hipSuccess)
		e = hipMalloc((void **)&b->t12, t12.size() * sizeof(float));
	if (e == hipSuccess)
		e = hipMalloc((void **)&b->steps, sizeof(steps));
	if (e == hipSuccess)
		e = hipMemsetAsync(b->rows, 0, (size_t)max_rows * sizeof(WrTonesRow), d->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(b->t12, t12.data(), t12.size() * sizeof(float), hipMemcpyHostToDevice, d->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(b->steps, steps, sizeof(steps), hipMemcpyHostToDevice, d->stream);
	return bank_created(bank, b, e, "wr_tones_create", wr_tones_destroy);
}

extern "C" int wr_tones_destroy(wr_tones *b)
{
	if (!b)
		return WR_OK;
	(void)hipSetDevice(b->dev->device);
	(void)wrc_dev_stream_sync(b->dev);
	(void)hipFree(b->rows);
	(void)hipFree(b->t12);
	(void)hipFree(b->steps);
	delete b;
	return WR_OK;
}

extern "C" int wr_tones_reset(wr_tones *b, int row)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_tones_reset: bank is NULL");
	size_t first, n;
	if (int rc = bank_reset_begin(b, "wr_tones_reset", row, &first, &n))
		return rc;
	/* a row that begins its stream is all zero: accumulators, latched result, window count and fill */
	HIP_TRY(hipMemsetAsync(b->rows + first, 0, n * sizeof(WrTonesRow), b->dev->stream));
	return WR_OK;
}

extern "C" int wr_tones_push_rows(wr_tones *b, const float *audio_dev, size_t row_stride, size_t nrows, size_t nframes)
{
	if (!b || !audio_dev)
		return wrc_fail(WR_ERR_ARG, "wr_tones_push_rows: bad argument (NULL bank or audio_dev)");
	if (int rc = bank_rows_refused(b, "wr_tones_push_rows", row_stride, nrows, nframes, 40))
		return rc;
	if (!nrows || !nframes)
		return WR_OK;
	if (int rc = bank_dev_ready(b->dev, true))
		return rc;
	HIP_TRY(wrk_tones_push(b->dev->stream, audio_dev, row_stride, nrows, nframes, b->rows, b->t12, b->steps, b->ntones, b->window));
	return WR_OK;
}

/* the last submit's audio rows of every channel slot into the bank: the rows wr_tuner_audio_dev shows, counted as
 * wr_tuner_chan_levels counts them, read where they lie */
extern "C" int wr_tuner_tones_push(wr_tuner *t, wr_tones *bank, unsigned int *slots)
{
	if (!t || !bank)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_tones_push: bad argument (NULL tuner or bank)");
	WrLastSubmit v;
	if (int rc = bank_take_submit(bank, "wr_tuner_tones_push", "bank", t, &v))
		return rc;
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	DEV_SETTLE(t->dev);
	const Group *g = v.g;
	if (v.used && g->last_k2)
		HIP_TRY(wrk_tones_push(t->dev->stream, g->dev.audio, g->k2max, v.used, g->last_k2, bank->rows, bank->t12, bank->steps,
		                       bank->ntones, bank->window));
	return bank_took_submit(bank, t, v, slots);
}

extern "C" int wr_tones_read(wr_tones *b, long long *iq_host, long long *energy_host, unsigned long long *windows_host,
                             unsigned int *fill_host, unsigned int *rows)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_tones_read: bank is NULL");
	if (!iq_host && !energy_host && !windows_host && !fill_host)
		return wrc_fail(WR_ERR_ARG, "wr_tones_read: no array to fill");
	wr_dev *d = b->dev;
	if (int rc = bank_dev_ready(d, false))
		return rc;
	const char *base = (const char *)b->rows;
	const size_t pitch = sizeof(WrTonesRow), n = b->max_rows;
	if (iq_host) {
		const size_t width = (size_t)b->ntones * 2u * sizeof(long long);
		HIP_TRY(hipMemcpy2DAsync(iq_host, width, base + offsetof(WrTonesRow, lat), pitch, width, n, hipMemcpyDeviceToHost, d->stream));
	}
	if (energy_host)
		HIP_TRY(hipMemcpy2DAsync(energy_host, sizeof(long long), base + offsetof(WrTonesRow, lat_e), pitch, sizeof(long long), n,
		                         hipMemcpyDeviceToHost, d->stream));
	if (windows_host)
		HIP_TRY(hipMemcpy2DAsync(windows_host, sizeof(unsigned long long), base + offsetof(WrTonesRow, windows), pitch,
		                         sizeof(unsigned long long), n, hipMemcpyDeviceToHost, d->stream));
	if (fill_host)
		HIP_TRY(hipMemcpy2DAsync(fill_host, sizeof(unsigned int), base + offsetof(WrTonesRow, fill), pitch, sizeof(unsigned int), n,
		                         hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	if (rows)
		*rows = b->max_rows;
	return WR_OK;
}

/* ------------------------------------------------------------------ DCS bank -- */

extern "C" int wr_dcs_word(unsigned int code, unsigned int *word)
{
	if (!word || code > 511u)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_word: word is NULL, or code %u (octal %o) is not inside 0 .. 511 (octal 777)", code, code);
	const unsigned int d = code | 0x800u;
	unsigned int p = d;
	for (unsigned int i = 0; i < 12u; ++i) {
		if (p & 1u)
			p ^= 0xC75u;
		p >>= 1;
	}
	*word = (p << 12) | d;
	return WR_OK;
}

static bool dcs_step_ok(unsigned long long step)
{
	return step >= (1ull << 19) && step <= (1ull << 28);
}

extern "C" int wr_dcs_step(unsigned int audio_rate, unsigned int *step)
{
	if (!step)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_step: step is NULL");
	const unsigned long long den = 5ull * audio_rate;
	const unsigned long long s = den ? ((672ull << 32) + den / 2u) / den : 0;
	if (!dcs_step_ok(s))
		return wrc_fail(WR_ERR_ARG, "wr_dcs_step: at %u Hz a chip (an eighth of a bit at 134.4 bit/s) is not 2 .. 1024 frames: the "
		                "step would be %llu, outside 2^19 .. 2^28", audio_rate, s);
	*step = (unsigned int)s;
	return WR_OK;
}

extern "C" int wr_dcs_create(wr_dcs **bank, wr_dev *d, unsigned int max_rows, const unsigned int *words_host, unsigned int ncodes,
                             unsigned int step, unsigned int max_errors)
{
	if (!bank || !words_host)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_create: bad argument (NULL bank or words_host)");
	if (!max_rows || max_rows > 65535u || !ncodes || ncodes > WR_DCS_CODES || !dcs_step_ok(step) || max_errors > 3u)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_create: %u rows (1 .. 65535), %u codes (1 .. 128), a step of %u (2^19 .. 2^28), "
		                "max_errors %u (0 .. 3)", max_rows, ncodes, step, max_errors);
	for (unsigned int k = 0; k < ncodes; ++k)
		if (words_host[k] >= (1u << 23))
			return wrc_fail(WR_ERR_ARG, "wr_dcs_create: code %u: the word 0x%x is not below 2^23", k, words_host[k]);
	if (!d)                                                     /* (behind the limits: those are refused without a device too) */
		return wrc_fail(WR_ERR_ARG, "wr_dcs_create: bad argument (NULL dev)");
	wr_dcs *b;
	if (int rc = bank_new(&b, "wr_dcs_create", d, max_rows))
		return rc;
	b->ncodes = ncodes;
	b->step = step;
	b->max_errors = max_errors;
	hipError_t e = hipMalloc((void **)&b->rows, (size_t)max_rows * sizeof(WrDcsRow));
	if (e == hipSuccess)
		e = hipMalloc((void **)&b->words, ncodes * sizeof(unsigned int));
	if (e == hipSuccess)
		e = hipMemsetAsync(b->rows, 0, (size_t)max_rows * sizeof(WrDcsRow), d->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(b->words, words_host, ncodes * sizeof(unsigned int), hipMemcpyHostToDevice, d->stream);
	return bank_created(bank, b, e, "wr_dcs_create", wr_dcs_destroy);
}

extern "C" int wr_dcs_destroy(wr_dcs *b)
{
	if (!b)
		return WR_OK;
	(void)hipSetDevice(b->dev->device);
	(void)wrc_dev_stream_sync(b->dev);
	(void)hipFree(b->rows);
	(void)hipFree(b->words);
	delete b;
	return WR_OK;
}

/* a reset of every row with the clock at `frame` */
static int dcs_restart(wr_dcs *b, const char *who, unsigned long long frame)
{
	size_t first, n;
	if (int rc = bank_reset_begin(b, who, -1, &first, &n))
		return rc;
	HIP_TRY(hipMemsetAsync(b->rows, 0, n * sizeof(WrDcsRow), b->dev->stream));
	b->zero_from = 0;
	b->frames = frame;
	return WR_OK;
}

extern "C" int wr_dcs_reset(wr_dcs *b, int row)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_reset: bank is NULL");
	if (row < 0)
		return dcs_restart(b, "wr_dcs_reset", 0);
	size_t first, n;
	if (int rc = bank_reset_begin(b, "wr_dcs_reset", row, &first, &n))
		return rc;
	/* a row that begins its stream is all zero: chips, the open one among them, agree, run, hits and evals; the clock runs on */
	HIP_TRY(hipMemsetAsync(b->rows + first, 0, n * sizeof(WrDcsRow), b->dev->stream));
	return WR_OK;
}

extern "C" int wr_dcs_seek(wr_dcs *b, unsigned long long frame)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_seek: bank is NULL");
	return dcs_restart(b, "wr_dcs_seek", frame);
}

/* the push itself, on a device made ready: the rows it leaves out are reset, the clock advances */
static int dcs_push(wr_dcs *b, const float *audio_dev, size_t row_stride, size_t nrows, size_t nframes)
{
	if (!nframes)
		return WR_OK;
	wr_dev *d = b->dev;
	if (nrows < b->zero_from)
		HIP_TRY(hipMemsetAsync(b->rows + nrows, 0, (b->zero_from - nrows) * sizeof(WrDcsRow), d->stream));
	HIP_TRY(wrk_dcs_push(d->stream, audio_dev, row_stride, nrows, nframes, b->rows, b->words, b->ncodes, b->step, b->frames,
	                     b->max_errors));
	b->zero_from = (unsigned int)nrows;
	b->frames += nframes;
	return WR_OK;
}

extern "C" int wr_dcs_push_rows(wr_dcs *b, const float *audio_dev, size_t row_stride, size_t nrows, size_t nframes)
{
	if (!b || !audio_dev)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_push_rows: bad argument (NULL bank or audio_dev)");
	if (int rc = bank_rows_refused(b, "wr_dcs_push_rows", row_stride, nrows, nframes, 28))
		return rc;
	if (!nframes)
		return WR_OK;
	if (int rc = bank_dev_ready(b->dev, true))
		return rc;
	return dcs_push(b, audio_dev, row_stride, nrows, nframes);
}

/* the rows wr_tuner_tones_push takes, into the DCS bank */
extern "C" int wr_tuner_dcs_push(wr_tuner *t, wr_dcs *bank, unsigned int *slots)
{
	if (!t || !bank)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_dcs_push: bad argument (NULL tuner or bank)");
	WrLastSubmit v;
	if (int rc = bank_take_submit(bank, "wr_tuner_dcs_push", "bank", t, &v))
		return rc;
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	DEV_SETTLE(t->dev);
	const Group *g = v.g;
	if (int rc = dcs_push(bank, g->dev.audio, g->k2max, v.used, g->last_k2))
		return rc;
	return bank_took_submit(bank, t, v, slots);
}

extern "C" int wr_dcs_read(wr_dcs *b, unsigned char *agree_host, unsigned int *run_host, unsigned long long *hits_host,
                           unsigned long long *evals_host, unsigned int *rows)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_read: bank is NULL");
	if (!agree_host && !run_host && !hits_host && !evals_host)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_read: no array to fill");
	wr_dev *d = b->dev;
	if (int rc = bank_dev_ready(d, false))
		return rc;
	const char *base = (const char *)b->rows;
	const size_t pitch = sizeof(WrDcsRow), n = b->max_rows, pairs = (size_t)b->ncodes * 2u;
	if (agree_host)
		HIP_TRY(hipMemcpy2DAsync(agree_host, pairs, base + offsetof(WrDcsRow, agree), pitch, pairs, n, hipMemcpyDeviceToHost,
		                         d->stream));
	if (run_host)
		HIP_TRY(hipMemcpy2DAsync(run_host, pairs * sizeof(unsigned int), base + offsetof(WrDcsRow, run), pitch,
		                         pairs * sizeof(unsigned int), n, hipMemcpyDeviceToHost, d->stream));
	if (hits_host)
		HIP_TRY(hipMemcpy2DAsync(hits_host, pairs * sizeof(unsigned long long), base + offsetof(WrDcsRow, hits), pitch,
		                         pairs * sizeof(unsigned long long), n, hipMemcpyDeviceToHost, d->stream));
	if (evals_host)
		HIP_TRY(hipMemcpy2DAsync(evals_host, sizeof(unsigned long long), base + offsetof(WrDcsRow, evals), pitch,
		                         sizeof(unsigned long long), n, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(wrc_dev_stream_sync(d));
	if (rows)
		*rows = b->max_rows;
	return WR_OK;
}

extern "C" int wr_dcs_info(wr_dcs *b, unsigned int *ncodes, unsigned int *step, unsigned int *max_errors, unsigned long long *frames)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_info: bank is NULL");
	if (ncodes)
		*ncodes = b->ncodes;
	if (step)
		*step = b->step;
	if (max_errors)
		*max_errors = b->max_errors;
	if (frames)
		*frames = b->frames;
	return WR_OK;
}

/* ------------------------------------------------------------------ resampler -- */

extern "C" int wr_resamp_ratio(unsigned int in_rate, unsigned int out_rate, unsigned int *L, unsigned int *M)
{
	if (!L || !M || wrd_resamp_ratio(in_rate, out_rate, L, M))
		return wrc_fail(WR_ERR_ARG, "wr_resamp_ratio: bad argument (NULL L or M, or a rate of 0: %u -> %u)", in_rate, out_rate);
	return WR_OK;
}

extern "C" int wr_resamp_design(unsigned int in_rate, unsigned int out_rate, unsigned int P, float *taps_host, unsigned int *L,
                                unsigned int *M)
{
	if (!taps_host)
		return wrc_fail(WR_ERR_ARG, "wr_resamp_design: taps_host is NULL");
	unsigned int l = 0, m = 0;
	if (wrd_resamp_design(in_rate, out_rate, P, taps_host, &l, &m))
		return wrc_fail(WR_ERR_ARG, "wr_resamp_design: %u -> %u Hz with %u taps per phase: a rate of 0, L / M outside 1 <= L <= 1024, "
		                "M <= 8 L, L <= 8 M, P not a multiple of 4 in 4 .. 64, L * P above 16384, or no passband "
		                "(min(in, out) <= 10 in / P)", in_rate, out_rate, P);
	if (L)
		*L = l;
	if (M)
		*M = m;
	return WR_OK;
}

extern "C" int wr_resamp_create(wr_resamp **rs, wr_dev *d, unsigned int max_rows, unsigned int L, unsigned int M, unsigned int P,
                                const float *taps_host)
{
	if (!rs || !d || !taps_host)
		return wrc_fail(WR_ERR_ARG, "wr_resamp_create: bad argument (NULL rs, dev or taps_host)");
	if (!max_rows || max_rows > 65535u || wrd_resamp_limits(L, M, P))
		return wrc_fail(WR_ERR_ARG, "wr_resamp_create: %u rows (1 .. 65535), L / M = %u / %u (1 <= L <= 1024, M <= 8 L, L <= 8 M), "
		                "%u taps per phase (a multiple of 4 in 4 .. 64, L * P <= 16384)", max_rows, L, M, P);
	const size_t ntaps = (size_t)L * P, nhist = (size_t)max_rows * (P - 1u);
	for (size_t i = 0; i < ntaps; ++i) {
		uint32_t bits;
		memcpy(&bits, taps_host + i, sizeof(bits));
		if ((bits & 0x7fffffffu) >= 0x7f800000u || !(fabsf(taps_host[i]) <= 16.0f))
			return wrc_fail(WR_ERR_ARG, "wr_resamp_create: tap [%zu][%zu] = %g is not finite or above 16 in magnitude", i / P, i % P,
			                (double)taps_host[i]);
	}
	wr_resamp *r;
	if (int rc = bank_new(&r, "wr_resamp_create", d, max_rows))
		return rc;
	r->L = L;
	r->M = M;
	r->P = P;
	hipError_t e = hipMalloc((void **)&r->taps, ntaps * sizeof(float));
	for (unsigned int s = 0; s < 2u && e == hipSuccess; ++s) {
		e = hipMalloc((void **)&r->hist[s], nhist * sizeof(float));
		if (e == hipSuccess)
			e = hipMemsetAsync(r->hist[s], 0, nhist * sizeof(float), d->stream);
	}
	if (e == hipSuccess)
		e = hipMemcpyAsync(r->taps, taps_host, ntaps * sizeof(float), hipMemcpyHostToDevice, d->stream);
	return bank_created(rs, r, e, "wr_resamp_create", wr_resamp_destroy);
}

extern "C" int wr_resamp_destroy(wr_resamp *r)
{
	if (!r)
		return WR_OK;
	(void)hipSetDevice(r->dev->device);
	(void)wrc_dev_stream_sync(r->dev);
	(void)hipFree(r->taps);
	(void)hipFree(r->hist[0]);
	(void)hipFree(r->hist[1]);
	delete r;
	return WR_OK;
}

extern "C" int wr_resamp_reset(wr_resamp *r, int row)
{
	if (!r)
		return wrc_fail(WR_ERR_ARG, "wr_resamp_reset: rs is NULL");
	size_t first, n;
	if (int rc = bank_reset_begin(r, "wr_resamp_reset", row, &first, &n))
		return rc;
	/* only the set the next push reads matters: that push writes the other one */
	const size_t H = r->P - 1u;
	HIP_TRY(hipMemsetAsync(r->hist[r->cur] + first * H, 0, n * H * sizeof(float), r->dev->stream));
	if (row < 0) {                                              /* all rows: the clock and the counts start again too */
		r->zero_from[r->cur] = 0;
		r->nmod = 0;
		r->frames_in = r->frames_out = 0;
	}
	return WR_OK;
}

extern "C" int wr_resamp_out_frames(wr_resamp *r, size_t nframes, size_t *n_out)
{
	if (!r || !n_out || nframes > ((size_t)1 << 28))
		return wrc_fail(WR_ERR_ARG, "wr_resamp_out_frames: bad argument (NULL rs or n_out, or more than 2^28 frames)");
	*n_out = (size_t)wrk_resamp_out_frames(r->L, r->M, r->nmod, nframes);
	return WR_OK;
}

/* what both pushes refuse, and the output frames of the push */
static int resamp_check(const wr_resamp *r, const char *who, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes,
                        const float *out_dev, size_t out_stride, size_t *n_out)
{
	if (int rc = bank_rows_refused(r, who, row_stride, nrows, nframes, 28))
		return rc;
	const size_t n = (size_t)wrk_resamp_out_frames(r->L, r->M, r->nmod, nframes);
	*n_out = n;
	if (!nrows || !n)
		return WR_OK;
	if (!out_dev || (nrows > 1 && out_stride < n))
		return wrc_fail(WR_ERR_ARG, "%s: out_dev is NULL, or rows of %zu output frames overlap at a stride of %zu", who, n, out_stride);
	const uintptr_t a0 = (uintptr_t)in_dev, a1 = a0 + ((nrows - 1u) * row_stride + nframes) * sizeof(float);
	const uintptr_t b0 = (uintptr_t)out_dev, b1 = b0 + ((nrows - 1u) * out_stride + n) * sizeof(float);
	if (a0 < b1 && b0 < a1)
		return wrc_fail(WR_ERR_ARG, "%s: input and output overlap", who);
	return WR_OK;
}

/* the push itself, behind resamp_check, on a device made ready: the rows it leaves out lose their histories, the clock and
 * the counts advance, the history sets change places */
static int resamp_push(wr_resamp *r, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                       size_t out_stride)
{
	if (!nframes)
		return WR_OK;
	wr_dev *d = r->dev;
	const unsigned int from = r->cur, to = from ^ 1u;
	const size_t H = r->P - 1u;
	if (nrows < r->zero_from[to])
		HIP_TRY(hipMemsetAsync(r->hist[to] + nrows * H, 0, (r->zero_from[to] - nrows) * H * sizeof(float), d->stream));
	const WrResampPush p = {r->taps, r->L, r->M, r->P, r->nmod, r->hist[from], r->hist[to]};
	HIP_TRY(wrk_resamp_push(d->stream, in_dev, row_stride, nrows, nframes, p, out_dev, out_stride));
	r->zero_from[to] = (unsigned int)nrows;
	r->cur = to;
	r->frames_in += nframes;
	r->frames_out += wrk_resamp_out_frames(r->L, r->M, r->nmod, nframes);
	r->nmod = (unsigned int)((r->nmod + nframes) % r->M);
	return WR_OK;
}

extern "C" int wr_resamp_push_rows(wr_resamp *r, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes,
                                   float *out_dev, size_t out_stride, size_t *n_out)
{
	if (!r || !in_dev || !n_out)
		return wrc_fail(WR_ERR_ARG, "wr_resamp_push_rows: bad argument (NULL rs, in_dev or n_out)");
	if (int rc = resamp_check(r, "wr_resamp_push_rows", in_dev, row_stride, nrows, nframes, out_dev, out_stride, n_out))
		return rc;
	if (!nframes)
		return WR_OK;
	if (int rc = bank_dev_ready(r->dev, true))
		return rc;
	return resamp_push(r, in_dev, row_stride, nrows, nframes, out_dev, out_stride);
}

/* the rows wr_tuner_tones_push takes, through the resampler: row s yields *n_out frames at out_dev + s * out_stride */
extern "C" int wr_tuner_resamp_push(wr_tuner *t, wr_resamp *rs, float *out_dev, size_t out_stride, size_t *n_out,
                                    unsigned int *slots)
{
	if (!t || !rs || !n_out)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_resamp_push: bad argument (NULL tuner, rs or n_out)");
	WrLastSubmit v;
	if (int rc = bank_take_submit(rs, "wr_tuner_resamp_push", "resampler", t, &v))
		return rc;
	const Group *g = v.g;
	if (int rc = resamp_check(rs, "wr_tuner_resamp_push", g->dev.audio, g->k2max, v.used, g->last_k2, out_dev, out_stride, n_out))
		return rc;
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	DEV_SETTLE(t->dev);
	if (int rc = resamp_push(rs, g->dev.audio, g->k2max, v.used, g->last_k2, out_dev, out_stride))
		return rc;
	return bank_took_submit(rs, t, v, slots);
}

extern "C" int wr_resamp_info(wr_resamp *r, unsigned int *L, unsigned int *M, unsigned int *P, unsigned long long *frames_in,
                              unsigned long long *frames_out)
{
	if (!r)
		return wrc_fail(WR_ERR_ARG, "wr_resamp_info: rs is NULL");
	if (L)
		*L = r->L;
	if (M)
		*M = r->M;
	if (P)
		*P = r->P;
	if (frames_in)
		*frames_in = r->frames_in;
	if (frames_out)
		*frames_out = r->frames_out;
	return WR_OK;
}

/* ------------------------------------------------------------------ voice bank -- */

extern "C" int wr_voice_design(unsigned int audio_rate, unsigned int T, unsigned int highpass_hz, unsigned int lowpass_hz,
                               unsigned int deemph_us, float *taps_host)
{
	if (!taps_host)
		return wrc_fail(WR_ERR_ARG, "wr_voice_design: taps_host is NULL");
	if (wrd_voice_design(audio_rate, T, highpass_hz, lowpass_hz, deemph_us, taps_host))
		return wrc_fail(WR_ERR_ARG, "wr_voice_design: %u taps at %u Hz, %u .. %u Hz, %u us: a rate of 0, T not a multiple of 4 in "
		                "8 .. 2048, an edge at or above half the rate, edges less than two transition half-widths (each about "
		                "3.84 rate / (T - 1) Hz) apart, or more than 10000 us", T, audio_rate, highpass_hz, lowpass_hz, deemph_us);
	return WR_OK;
}

extern "C" int wr_voice_create(wr_voice **bank, wr_dev *d, unsigned int max_rows, unsigned int T, unsigned int nfilt,
                               const float *taps_host)
{
	if (!bank || !taps_host)
		return wrc_fail(WR_ERR_ARG, "wr_voice_create: bad argument (NULL bank or taps_host)");
	if (!max_rows || max_rows > 65535u || !wrp_voice_len_ok(T) || !nfilt || nfilt > VOICE_FILTERS)
		return wrc_fail(WR_ERR_ARG, "wr_voice_create: %u rows (1 .. 65535), %u taps (a multiple of 4 in 8 .. 2048), %u filters "
		                "(1 .. 16)", max_rows, T, nfilt);
	const size_t ntaps = (size_t)nfilt * T, nhist = (size_t)max_rows * (T - 1u);
	for (size_t i = 0; i < ntaps; ++i) {
		uint32_t bits;
		memcpy(&bits, taps_host + i, sizeof(bits));
		if ((bits & 0x7fffffffu) >= 0x7f800000u || !(fabsf(taps_host[i]) <= 16.0f))
			return wrc_fail(WR_ERR_ARG, "wr_voice_create: tap [%zu][%zu] = %g is not finite or above 16 in magnitude", i / T, i % T,
			                (double)taps_host[i]);
	}
	if (!d)                                                     /* (behind the limits: those are refused without a device too) */
		return wrc_fail(WR_ERR_ARG, "wr_voice_create: bad argument (NULL dev)");
	wr_voice *b;
	if (int rc = bank_new(&b, "wr_voice_create", d, max_rows))
		return rc;
	b->T = T;
	b->nfilt = nfilt;
	b->ctl_host = (unsigned int *)calloc(max_rows, sizeof(unsigned int));
	hipError_t e = b->ctl_host ? hipMalloc((void **)&b->taps, ntaps * sizeof(float)) : hipErrorOutOfMemory;
	if (e == hipSuccess)
		e = hipMalloc((void **)&b->ctl, (size_t)max_rows * sizeof(unsigned int));
	if (e == hipSuccess)
		e = hipMemsetAsync(b->ctl, 0, (size_t)max_rows * sizeof(unsigned int), d->stream);
	for (unsigned int s = 0; s < 2u && e == hipSuccess; ++s) {
		e = hipMalloc((void **)&b->hist[s], nhist * sizeof(float));
		if (e == hipSuccess)
			e = hipMemsetAsync(b->hist[s], 0, nhist * sizeof(float), d->stream);
	}
	if (e == hipSuccess)
		e = hipMemcpyAsync(b->taps, taps_host, ntaps * sizeof(float), hipMemcpyHostToDevice, d->stream);
	return bank_created(bank, b, e, "wr_voice_create", wr_voice_destroy);
}

extern "C" int wr_voice_destroy(wr_voice *b)
{
	if (!b)
		return WR_OK;
	(void)hipSetDevice(b->dev->device);
	(void)wrc_dev_stream_sync(b->dev);
	(void)hipFree(b->taps);
	(void)hipFree(b->ctl);
	(void)hipFree(b->hist[0]);
	(void)hipFree(b->hist[1]);
	free(b->ctl_host);
	delete b;
	return WR_OK;
}

extern "C" int wr_voice_reset(wr_voice *b, int row)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_voice_reset: bank is NULL");
	size_t first, n;
	if (int rc = bank_reset_begin(b, "wr_voice_reset", row, &first, &n))
		return rc;
	/* only the set the next push reads matters: that push writes the other one; the control words stay */
	const size_t H = b->T - 1u;
	HIP_TRY(hipMemsetAsync(b->hist[b->cur] + first * H, 0, n * H * sizeof(float), b->dev->stream));
	if (row < 0) {                                              /* all rows: the frame count starts again too */
		b->zero_from[b->cur] = 0;
		b->frames = 0;
	}
	return WR_OK;
}

/* rows [first, first + n) are the bank's */
static int voice_rows_in_range(const wr_voice *b, const char *who, unsigned int first, unsigned int n)
{
	if (first > b->max_rows || n > b->max_rows - first)
		return wrc_fail(WR_ERR_ARG, "%s: rows %u .. %u of a bank of %u", who, first, first + n, b->max_rows);
	return WR_OK;
}

extern "C" int wr_voice_set_rows(wr_voice *b, unsigned int first, unsigned int n, const unsigned int *ctl_host)
{
	if (!b || !ctl_host)
		return wrc_fail(WR_ERR_ARG, "wr_voice_set_rows: bad argument (NULL bank or ctl_host)");
	if (int rc = voice_rows_in_range(b, "wr_voice_set_rows", first, n))
		return rc;
	for (unsigned int r = 0; r < n; ++r)                        /* every word, before any changes */
		if ((ctl_host[r] & ~0x1ffu) || (ctl_host[r] & 0xffu) >= b->nfilt)
			return wrc_fail(WR_ERR_ARG, "wr_voice_set_rows: row %u: the word 0x%x names filter %u of %u, or has a bit set beyond the "
			                "filter index (bits 0-7) and mute (bit 8)", first + r, ctl_host[r], ctl_host[r] & 0xffu, b->nfilt);
	if (!n)
		return WR_OK;
	if (int rc = bank_dev_ready(b->dev, false))
		return rc;
	/* on the stream, behind the pushes already there, and waited for: the source is the caller's */
	HIP_TRY(hipMemcpyAsync(b->ctl + first, ctl_host, (size_t)n * sizeof(unsigned int), hipMemcpyHostToDevice, b->dev->stream));
	HIP_TRY(wrc_dev_stream_sync(b->dev));
	memcpy(b->ctl_host + first, ctl_host, (size_t)n * sizeof(unsigned int));
	return WR_OK;
}

extern "C" int wr_voice_get_rows(wr_voice *b, unsigned int first, unsigned int n, unsigned int *ctl_host)
{
	if (!b || !ctl_host)
		return wrc_fail(WR_ERR_ARG, "wr_voice_get_rows: bad argument (NULL bank or ctl_host)");
	if (int rc = voice_rows_in_range(b, "wr_voice_get_rows", first, n))
		return rc;
	memcpy(ctl_host, b->ctl_host + first, (size_t)n * sizeof(unsigned int));
	return WR_OK;
}

/* what both pushes refuse */
static int voice_check(const wr_voice *b, const char *who, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes,
                       const float *out_dev, size_t out_stride)
{
	if (int rc = bank_rows_refused(b, who, row_stride, nrows, nframes, 28))
		return rc;
	if (!nrows || !nframes)
		return WR_OK;
	if (!out_dev || (nrows > 1 && out_stride < nframes))
		return wrc_fail(WR_ERR_ARG, "%s: out_dev is NULL, or rows of %zu output frames overlap at a stride of %zu", who, nframes,
		                out_stride);
	const uintptr_t a0 = (uintptr_t)in_dev, a1 = a0 + ((nrows - 1u) * row_stride + nframes) * sizeof(float);
	const uintptr_t b0 = (uintptr_t)out_dev, b1 = b0 + ((nrows - 1u) * out_stride + nframes) * sizeof(float);
	if (a0 < b1 && b0 < a1)
		return wrc_fail(WR_ERR_ARG, "%s: input and output overlap", who);
	return WR_OK;
}

/* the push itself, behind voice_check, on a device made ready: the rows it leaves out lose their histories, the count
 * advances, the history sets change places */
static int voice_push(wr_voice *b, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                      size_t out_stride)
{
	if (!nframes)
		return WR_OK;
	wr_dev *d = b->dev;
	const unsigned int from = b->cur, to = from ^ 1u;
	const size_t H = b->T - 1u;
	if (nrows < b->zero_from[to])
		HIP_TRY(hipMemsetAsync(b->hist[to] + nrows * H, 0, (b->zero_from[to] - nrows) * H * sizeof(float), d->stream));
	const WrVoicePush p = {b->taps, b->T, b->ctl, b->hist[from], b->hist[to]};
	HIP_TRY(wrk_voice_push(d->stream, in_dev, row_stride, nrows, nframes, p, out_dev, out_stride));
	b->zero_from[to] = (unsigned int)nrows;
	b->cur = to;
	b->frames += nframes;
	return WR_OK;
}

extern "C" int wr_voice_push_rows(wr_voice *b, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                                  size_t out_stride)
{
	if (!b || !in_dev)
		return wrc_fail(WR_ERR_ARG, "wr_voice_push_rows: bad argument (NULL bank or in_dev)");
	if (int rc = voice_check(b, "wr_voice_push_rows", in_dev, row_stride, nrows, nframes, out_dev, out_stride))
		return rc;
	if (!nframes)
		return WR_OK;
	if (int rc = bank_dev_ready(b->dev, true))
		return rc;
	return voice_push(b, in_dev, row_stride, nrows, nframes, out_dev, out_stride);
}

/* the rows wr_tuner_resamp_push takes, through the voice bank: row s yields the submit's audio frames at out_dev + s * out_stride */
extern "C" int wr_tuner_voice_push(wr_tuner *t, wr_voice *bank, float *out_dev, size_t out_stride, unsigned int *slots)
{
	if (!t || !bank)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_voice_push: bad argument (NULL tuner or bank)");
	WrLastSubmit v;
	if (int rc = bank_take_submit(bank, "wr_tuner_voice_push", "bank", t, &v))
		return rc;
	const Group *g = v.g;
	if (int rc = voice_check(bank, "wr_tuner_voice_push", g->dev.audio, g->k2max, v.used, g->last_k2, out_dev, out_stride))
		return rc;
	if (int rc = wrc_last_submit_flush(t, &v))
		return rc;
	DEV_SETTLE(t->dev);
	if (int rc = voice_push(bank, g->dev.audio, g->k2max, v.used, g->last_k2, out_dev, out_stride))
		return rc;
	return bank_took_submit(bank, t, v, slots);
}

extern "C" int wr_voice_info(wr_voice *b, unsigned int *T, unsigned int *nfilt, unsigned long long *frames)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "wr_voice_info: bank is NULL");
	if (T)
		*T = b->T;
	if (nfilt)
		*nfilt = b->nfilt;
	if (frames)
		*frames = b->frames;
	return WR_OK;
}
