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

/* ... its middle, behind the bank's own refusals: the submit's audio is there and no streaming launch is open on the device ... */
static int bank_submit_ready(wr_tuner *t, WrLastSubmit *v)
{
	if (int rc = wrc_last_submit_flush(t, v))
		return rc;
	return wrc_dev_settle_stream(t->dev);
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

/* a destroy's first steps; false: there is no bank */
static bool bank_destroy_begin(const WrRowBank *b)
{
	if (!b)
		return false;
	(void)hipSetDevice(b->dev->device);
	(void)wrc_dev_stream_sync(b->dev);
	return true;
}

/* a read's first steps (`any`: the caller gave an array to fill) ... */
static int bank_read_begin(const WrRowBank *b, const char *who, bool any)
{
	if (!b)
		return wrc_fail(WR_ERR_ARG, "%s: bank is NULL", who);
	if (!any)
		return wrc_fail(WR_ERR_ARG, "%s: no array to fill", who);
	return bank_dev_ready(b->dev, false);
}

/* ... one member of every row (`width` bytes at `offset` of rows `pitch` bytes apart) into the caller's array, if there is one ... */
static hipError_t bank_read_column(const WrRowBank *b, void *host, const void *rows, size_t pitch, size_t offset, size_t width)
{
	if (!host)
		return hipSuccess;
	return hipMemcpy2DAsync(host, width, (const char *)rows + offset, pitch, width, b->max_rows, hipMemcpyDeviceToHost, b->dev->stream);
}

/* ... and its last */
static int bank_read_end(const WrRowBank *b, unsigned int *rows)
{
	HIP_TRY(wrc_dev_stream_sync(b->dev));
	if (rows)
		*rows = b->max_rows;
	return WR_OK;
}

/* a filter table [nsets][len] as a create takes it: every tap finite and 16 at most in magnitude */
static int bank_taps_refused(const char *who, const float *taps_host, size_t nsets, size_t len)
{
	for (size_t i = 0; i < nsets * len; ++i) {
		uint32_t bits;
		memcpy(&bits, taps_host + i, sizeof(bits));
		if ((bits & 0x7fffffffu) >= 0x7f800000u || !(fabsf(taps_host[i]) <= 16.0f))
			return wrc_fail(WR_ERR_ARG, "%s: tap [%zu][%zu] = %g is not finite or above 16 in magnitude", who, i / len, i % len,
			                (double)taps_host[i]);
	}
	return WR_OK;
}

/* what a push that writes rows of `n_out` frames refuses of its output: none, rows that overlap, rows that overlap the input */
static int bank_out_refused(const char *who, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes,
                            const float *out_dev, size_t out_stride, size_t n_out)
{
	if (!nrows || !n_out)
		return WR_OK;
	if (!out_dev || (nrows > 1 && out_stride < n_out))
		return wrc_fail(WR_ERR_ARG, "%s: out_dev is NULL, or rows of %zu output frames overlap at a stride of %zu", who, n_out, out_stride);
	const uintptr_t a0 = (uintptr_t)in_dev, a1 = a0 + ((nrows - 1u) * row_stride + nframes) * sizeof(float);
	const uintptr_t b0 = (uintptr_t)out_dev, b1 = b0 + ((nrows - 1u) * out_stride + n_out) * sizeof(float);
	if (a0 < b1 && b0 < a1)
		return wrc_fail(WR_ERR_ARG, "%s: input and output overlap", who);
	return WR_OK;
}

/* ---- the two history sets of the resampler and the voice bank (WrHistSets) ---- */

/* both sets for `rows` rows of `H` frames, silent */
static hipError_t hist_alloc(WrHistSets *h, size_t rows, size_t H, hipStream_t st)
{
	hipError_t e = hipSuccess;
	h->H = H;
	for (unsigned int s = 0; s < 2u && e == hipSuccess; ++s) {
		e = hipMalloc((void **)&h->set[s], rows * H * sizeof(float));
		if (e == hipSuccess)
			e = hipMemsetAsync(h->set[s], 0, rows * H * sizeof(float), st);
	}
	return e;
}

static void hist_free(WrHistSets *h)
{
	(void)hipFree(h->set[0]);
	(void)hipFree(h->set[1]);
}

/* rows [first, first + n) begin their streams (`all`: they are all of the bank's).  Only the set the next push reads
 * matters: that push writes the other one */
static hipError_t hist_reset(WrHistSets *h, size_t first, size_t n, bool all, hipStream_t st)
{
	const hipError_t e = hipMemsetAsync(h->set[h->cur] + first * h->H, 0, n * h->H * sizeof(float), st);
	if (e == hipSuccess && all)
		h->zero_from[h->cur] = 0;
	return e;
}

/* a push of `nrows` rows reads *from and writes *to, where the rows it leaves out lose their histories */
static hipError_t hist_push_begin(WrHistSets *h, size_t nrows, hipStream_t st, const float **from, float **to)
{
	const unsigned int w = h->cur ^ 1u;
	*from = h->set[h->cur];
	*to = h->set[w];
	if (nrows >= h->zero_from[w])
		return hipSuccess;
	return hipMemsetAsync(h->set[w] + nrows * h->H, 0, (h->zero_from[w] - nrows) * h->H * sizeof(float), st);
}

/* ... and once it has gone out the sets change places */
static void hist_push_end(WrHistSets *h, size_t nrows)
{
	h->cur ^= 1u;
	h->zero_from[h->cur] = (unsigned int)nrows;
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
	if (!max_rows || max_rows > 65535u || !ntones || ntones > WR_LANES || window < TN_WINDOW_MIN || window > TN_WINDOW_MAX)
		return wrc_fail(WR_ERR_ARG, "wr_tones_create: %u rows (1 .. 65535), %u tones (1 .. 64), a window of %u frames "
		                "(16 .. 65536)", max_rows, ntones, window);
	unsigned int steps[WR_LANES] = {0};
	for (unsigned int t = 0; t < ntones; ++t) {
		if (!steps_host[t] || steps_host[t] >= 0x80000000u)
			return wrc_fail(WR_ERR_ARG, "wr_tones_create: tone %u: a step of %u is not inside (0, 2^31)", t, steps_host[t]);
		steps[t] = steps_host[t];
	}
	std::vector<float> table(WR_TABLE_SIZE), t12(TN_TABLE);
	wrd_sin_table(table.data());
	for (unsigned int i = 0; i < TN_TABLE; ++i)
		t12[i] = table[WR_TABLE_SIZE / TN_TABLE * i];
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
	if (!bank_destroy_begin(b))
		return WR_OK;
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
	if (int rc = bank_submit_ready(t, &v))
		return rc;
	const Group *g = v.g;
	HIP_TRY(wrk_tones_push(t->dev->stream, g->dev.audio, g->k2max, v.used, g->last_k2, bank->rows, bank->t12, bank->steps,
	                       bank->ntones, bank->window));
	return bank_took_submit(bank, t, v, slots);
}

extern "C" int wr_tones_read(wr_tones *b, long long *iq_host, long long *energy_host, unsigned long long *windows_host,
                             unsigned int *fill_host, unsigned int *rows)
{
	if (int rc = bank_read_begin(b, "wr_tones_read", iq_host || energy_host || windows_host || fill_host))
		return rc;
	const size_t pitch = sizeof(WrTonesRow);
	HIP_TRY(bank_read_column(b, iq_host, b->rows, pitch, offsetof(WrTonesRow, lat), (size_t)b->ntones * 2u * sizeof(long long)));
	HIP_TRY(bank_read_column(b, energy_host, b->rows, pitch, offsetof(WrTonesRow, lat_e), sizeof(long long)));
	HIP_TRY(bank_read_column(b, windows_host, b->rows, pitch, offsetof(WrTonesRow, windows), sizeof(unsigned long long)));
	HIP_TRY(bank_read_column(b, fill_host, b->rows, pitch, offsetof(WrTonesRow, fill), sizeof(unsigned int)));
	return bank_read_end(b, rows);
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

extern "C" int wr_dcs_step(unsigned int audio_rate, unsigned int *step)
{
	if (!step)
		return wrc_fail(WR_ERR_ARG, "wr_dcs_step: step is NULL");
	const unsigned long long den = 5ull * audio_rate;
	const unsigned long long s = den ? ((672ull << 32) + den / 2u) / den : 0;
	if (!wrp_dcs_step_ok(s))
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
	if (!max_rows || max_rows > 65535u || !ncodes || ncodes > WR_DCS_CODES || !wrp_dcs_step_ok(step) || max_errors > 3u)
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
	if (!bank_destroy_begin(b))
		return WR_OK;
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
	if (int rc = bank_submit_ready(t, &v))
		return rc;
	const Group *g = v.g;
	if (int rc = dcs_push(bank, g->dev.audio, g->k2max, v.used, g->last_k2))
		return rc;
	return bank_took_submit(bank, t, v, slots);
}

extern "C" int wr_dcs_read(wr_dcs *b, unsigned char *agree_host, unsigned int *run_host, unsigned long long *hits_host,
                           unsigned long long *evals_host, unsigned int *rows)
{
	if (int rc = bank_read_begin(b, "wr_dcs_read", agree_host || run_host || hits_host || evals_host))
		return rc;
	const size_t pitch = sizeof(WrDcsRow), pairs = (size_t)b->ncodes * 2u;
	HIP_TRY(bank_read_column(b, agree_host, b->rows, pitch, offsetof(WrDcsRow, agree), pairs));
	HIP_TRY(bank_read_column(b, run_host, b->rows, pitch, offsetof(WrDcsRow, run), pairs * sizeof(unsigned int)));
	HIP_TRY(bank_read_column(b, hits_host, b->rows, pitch, offsetof(WrDcsRow, hits), pairs * sizeof(unsigned long long)));
	HIP_TRY(bank_read_column(b, evals_host, b->rows, pitch, offsetof(WrDcsRow, evals), sizeof(unsigned long long)));
	return bank_read_end(b, rows);
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
	const size_t ntaps = (size_t)L * P;
	if (int rc = bank_taps_refused("wr_resamp_create", taps_host, L, P))
		return rc;
	wr_resamp *r;
	if (int rc = bank_new(&r, "wr_resamp_create", d, max_rows))
		return rc;
	r->L = L;
	r->M = M;
	r->P = P;
	hipError_t e = hipMalloc((void **)&r->taps, ntaps * sizeof(float));
	if (e == hipSuccess)
		e = hist_alloc(&r->hist, max_rows, P - 1u, d->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(r->taps, taps_host, ntaps * sizeof(float), hipMemcpyHostToDevice, d->stream);
	return bank_created(rs, r, e, "wr_resamp_create", wr_resamp_destroy);
}

extern "C" int wr_resamp_destroy(wr_resamp *r)
{
	if (!bank_destroy_begin(r))
		return WR_OK;
	(void)hipFree(r->taps);
	hist_free(&r->hist);
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
	HIP_TRY(hist_reset(&r->hist, first, n, row < 0, r->dev->stream));
	if (row < 0) {                                              /* all rows: the clock and the counts start again too */
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
	*n_out = (size_t)wrk_resamp_out_frames(r->L, r->M, r->nmod, nframes);
	return bank_out_refused(who, in_dev, row_stride, nrows, nframes, out_dev, out_stride, *n_out);
}

/* the push itself, behind resamp_check, on a device made ready: the rows it leaves out lose their histories, the clock and
 * the counts advance, the history sets change places */
static int resamp_push(wr_resamp *r, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                       size_t out_stride)
{
	if (!nframes)
		return WR_OK;
	wr_dev *d = r->dev;
	WrResampPush p = {r->taps, r->L, r->M, r->P, r->nmod, nullptr, nullptr};
	HIP_TRY(hist_push_begin(&r->hist, nrows, d->stream, &p.hist_old, &p.hist_new));
	HIP_TRY(wrk_resamp_push(d->stream, in_dev, row_stride, nrows, nframes, p, out_dev, out_stride));
	hist_push_end(&r->hist, nrows);
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
	if (int rc = bank_submit_ready(t, &v))
		return rc;
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
	const size_t ntaps = (size_t)nfilt * T;
	if (int rc = bank_taps_refused("wr_voice_create", taps_host, nfilt, T))
		return rc;
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
	if (e == hipSuccess)
		e = hist_alloc(&b->hist, max_rows, T - 1u, d->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(b->taps, taps_host, ntaps * sizeof(float), hipMemcpyHostToDevice, d->stream);
	return bank_created(bank, b, e, "wr_voice_create", wr_voice_destroy);
}

extern "C" int wr_voice_destroy(wr_voice *b)
{
	if (!bank_destroy_begin(b))
		return WR_OK;
	(void)hipFree(b->taps);
	(void)hipFree(b->ctl);
	hist_free(&b->hist);
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
	HIP_TRY(hist_reset(&b->hist, first, n, row < 0, b->dev->stream));      /* (the control words stay) */
	if (row < 0)                                                /* all rows: the frame count starts again too */
		b->frames = 0;
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
	return bank_out_refused(who, in_dev, row_stride, nrows, nframes, out_dev, out_stride, nframes);
}

/* the push itself, behind voice_check, on a device made ready: the rows it leaves out lose their histories, the count
 * advances, the history sets change places */
static int voice_push(wr_voice *b, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                      size_t out_stride)
{
	if (!nframes)
		return WR_OK;
	wr_dev *d = b->dev;
	WrVoicePush p = {b->taps, b->T, b->ctl, nullptr, nullptr};
	HIP_TRY(hist_push_begin(&b->hist, nrows, d->stream, &p.hist_old, &p.hist_new));
	HIP_TRY(wrk_voice_push(d->stream, in_dev, row_stride, nrows, nframes, p, out_dev, out_stride));
	hist_push_end(&b->hist, nrows);
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
	if (int rc = bank_submit_ready(t, &v))
		return rc;
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
