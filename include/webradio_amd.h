/*
 * webradio_amd.h -- C ABI of the MI355X (gfx950) backend for webradio's per-tuner
 * DSP hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI: its "plugin" interface
 * is the C++ virtual operator DspBlock (init/deinit/process, dsp/dspblock.h:82-84)
 * and the setters its callers use.  Each entry point below replaces the body of
 * one of those members; the host-side classes in webradio_amd/host/ keep the
 * reference's class names and signatures and forward to these functions, so
 * radio.cxx compiles against them unchanged (INTEGRATION.md shows the stub a
 * webradio maintainer would add to the upstream classes instead).
 *
 * Conventions
 *   - plain C, opaque handles, caller-owned buffers with explicit sizes
 *   - every function returns WR_OK (0) or a WR_ERR_* code; wr_last_error() gives a
 *     thread-local message.  The host classes map != WR_OK to `return false`
 *     from init()/process(), which is the reference's only error channel
 *     (dspblock.cxx:114-117,192-195).
 *   - "frames" are IQ pairs (one sample instant); IQ is interleaved float32
 *     [I0,Q0,I1,Q1,...] exactly like the reference's vector<sample_t> buffers.
 *   - pointers named *_dev are HIP device pointers on the context's device;
 *     pointers named *_host are ordinary host memory.
 *   - all work of one wr_dev is issued on one HIP stream given by the caller (e.g.
 *     torch.cuda.current_stream().cuda_stream); NULL is HIP's default stream.
 *     Functions taking host pointers synchronise that stream before returning;
 *     functions taking only device pointers are asynchronous.
 *   - there is NO CPU fallback: without a GPU wr_dev_open fails with
 *     WR_ERR_NODEV and nothing else can be created.
 *
 * Reference paths are relative to webradio's src/.
 */
#ifndef WEBRADIO_AMD_H_
#define WEBRADIO_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WR_ABI_VERSION   6       /* 2: wr_tuner_seek, *_n filters, af_gain/squelch, async uploads, ring_ready,
                                    blocks per launch added.  3: wr_ring_* (the halo ring of a time-sharded stream, incl.
                                    wr_ring_exchange_after / wr_tuner_mark_launches), wr_u8_to_f32_from_host, wr_dev_upload_ahead,
                                    wr_dev_wait_uploads_but added; channel filters of 128 / 256 taps accepted (WR_FIR_FUSED_MAX).
                                    4: wr_tune, wr_stage_windows_from_host, wr_tuner_last_staging added.
                                    5: wr_tuner_set_streaming, wr_tuner_stream_info, wr_block_kernel_calls added; audio filters and second
                                    channel stages of 128 / 256 taps accepted.
                                    6: wr_spectrum_lazy_info, wr_tuner_stream_host_blocks, wr_tuner_stream_long_blocks, wr_tuner_submit_count, WR_STREAM_MAX_BLOCKS added; wr_tuner_set_streaming
                                    takes 2 (byte blocks out of page-locked host memory stream too), wr_tuner_last_staging may say 3;
                                    wr_spectrum_push beside an open streaming launch keeps the frame and transforms it on demand.
                                    Added to 6 later: wr_spectrum_create_real, wr_spectrum_channels, wr_spectrum_batch_db_rows.
                                    Added to 6 later: wr_tuner_chan_spectra.
                                    Added to 6 later: wr_tuner_chan_levels, wr_iq_levels.
                                    Added to 6 later: wr_agc_design, wr_agc_rows, wr_chan_set_agc, wr_chan_get_agc, wr_tuner_agc_info.
                                    Added to 6 later: wr_tone_step, wr_tones_create, wr_tones_destroy, wr_tones_reset,
                                                      wr_tones_push_rows, wr_tuner_tones_push, wr_tones_read.
                                    Added to 6 later: wr_resamp_ratio, wr_resamp_design, wr_resamp_create, wr_resamp_destroy,
                                                      wr_resamp_reset, wr_resamp_out_frames, wr_resamp_push_rows,
                                                      wr_resamp_info, wr_tuner_resamp_push.
                                    Added to 6 later: wr_dcs_word, wr_dcs_step, wr_dcs_create, wr_dcs_destroy, wr_dcs_reset,
                                                      wr_dcs_seek, wr_dcs_push_rows, wr_tuner_dcs_push, wr_dcs_read, wr_dcs_info.
                                    Added to 6 later: wr_spectrum_batch_avg, wr_spectrum_rows_waterfall.
                                    Added to 6 later: wr_detect_rule_default, wr_spectrum_bin_hz, wr_spectrum_rows_detect.
                                    Added to 6 later: wr_voice_design, wr_voice_create, wr_voice_destroy, wr_voice_reset,
                                                      wr_voice_set_rows, wr_voice_get_rows, wr_voice_push_rows,
                                                      wr_tuner_voice_push, wr_voice_info.
                                    Nothing of an earlier version changed or removed */
#define WR_FIR_LENGTH    64      /* dsp/lowpass.cxx:39  FIR_LENGTH */
#define WR_TABLE_SIZE    65536   /* dsp/downconverter.cxx:35 LOOKUP_BITS 16 */

enum wr_status {
	WR_OK = 0,
	WR_ERR_ARG = 1,          /* bad argument (NULL, size, not a power of two, ...) */
	WR_ERR_HIP = 2,          /* a HIP runtime call or kernel launch failed */
	WR_ERR_STATE = 3,        /* call not legal in this state */
	WR_ERR_NOMEM = 4,
	WR_ERR_NODEV = 5,        /* no usable gfx950 device: the product has no CPU path */
	WR_ERR_RATE = 6          /* rates not integer related (dspblock.cxx:119-130) */
};

/* dsp/demodulator.h:40-46 enum Mode, same numbering */
enum wr_mode { WR_AM = 0, WR_FM = 1, WR_USB = 2, WR_LSB = 3 };

/* pipeline stages of one receiver chain (radio.cxx:68-76) that can be fetched */
enum wr_stage {
	WR_STAGE_CHAN_IQ = 1,    /* output of Receiver::_channelFilter  (2 ch) */
	WR_STAGE_DEMOD   = 2,    /* output of Receiver::_demodulator    (1 ch) */
	WR_STAGE_AUDIO   = 3     /* output of Receiver::_audioFilter    (1 ch) */
};

/* how the NCO sine/cosine of dsp/downconverter.cxx:100-101 is obtained */
enum wr_nco {
	WR_NCO_SPLIT = 0,        /* exact integer phase, sin/cos from two 256-entry
	                            LDS tables (coarse x fine angle addition); LO within
	                            3.5e-7 of the reference table entry */
	WR_NCO_EXACT = 1,        /* the reference's own 65536-entry sinf table, gathered from
	                            global memory, unfused multiply/add in the reference's
	                            order: channel-filter output is bit-identical */
	WR_NCO_ROTATE = 2        /* what the host runtime and bench.py use: the same table index sequence as the reference (exact integer
	                            phase), but each LO value is reached by turning the previous
	                            one by one of the two table angles the step allows, folded
	                            into the FIR as a Horner recurrence: no table access per tap.
	                            Channel IQ within 2e-7 of the bit-exact path for |x| <= 1 */
};

enum wr_where { WR_HOST = 0, WR_DEVICE = 1 };

typedef struct wr_dev      wr_dev;
typedef struct wr_tuner    wr_tuner;
typedef struct wr_spectrum wr_spectrum;
typedef struct wr_ring     wr_ring;
typedef struct wr_tones    wr_tones;
typedef struct wr_resamp   wr_resamp;
typedef struct wr_dcs      wr_dcs;
typedef struct wr_voice    wr_voice;

/* ------------------------------------------------------------------ misc -- */
int         wr_abi_version(void);
const char *wr_last_error(void);
int         wr_device_count(int *count);
/* Launch heuristics of the library, process-wide; they never change a result, only which of several
 * bit-identical kernel variants a launch takes.  Sets `key` to `value` (value < 0: back to the built-in /
 * environment default) and stores the value it had in *previous (optional).  For tests (both variants on
 * streams too short to reach a threshold) and for tuning; the reference has no counterpart. */
enum wr_tunable {
	WR_TUNE_DDC_NG2_MIN_PASSES = 1   /* k_tuner_ddc runs two lane groups per wave from this many passes of the grid on
	                                    (default 4, or $WR_DDC_NG2_MIN_PASSES at first use); 0: whenever the launch allows */
};
int         wr_tune(int key, long value, long *previous);

/* --------------------------------------------- host-side design helpers -- */
/* DownConverter::init / setIF: phaseStep = (int)((int64)hz * 2^31 / (int64)rate)
 * (dsp/downconverter.cxx:65,80) */
int wr_phase_step(int if_hz, unsigned int input_rate, int *phase_step);
/* DownConverter ctor table (dsp/downconverter.cxx:49-51); table[65536] */
int wr_sin_table(float *table_host);
/* LowPass::init window + LowPass::recalculate (dsp/lowpass.cxx:104-110,164-189):
 * 64 taps for `passband` Hz at `input_rate`; *maxbin_out (optional) receives the
 * integer cut-off bin of lowpass.cxx:167 */
int wr_lowpass_design(unsigned int passband, unsigned int input_rate,
                      float *coeff_host /* [64] */, unsigned int *maxbin_out);
/* the same with LowPass::_firLength = fir_length instead of the compiled-in 64: the
 * reference's FIXME "Make runtime variable" (dsp/lowpass.cxx:38-39) acted on -- every
 * expression of init()/recalculate() is already written in terms of _firLength.  A power of
 * two (the mask logic of lowpass.cxx:172,184) in [2, WR_FIR_MAX]. */
#define WR_FIR_MAX 1024
#define WR_FIR_FUSED_MAX 256     /* longest filter the per-tuner path takes (wr_chan_set_taps_n; r05: any of the three stages) */
int wr_lowpass_design_n(unsigned int fir_length, unsigned int passband, unsigned int input_rate,
                        float *coeff_host /* [fir_length] */, unsigned int *maxbin_out);
/* SpectrumSink::init window (io/spectrumsink.cxx:71-74); window[fft_size] */
int wr_spectrum_window(unsigned int fft_size, float *window_host);

/* ---------------------------------------------------------- device ctx -- */
/* Binds a device and a stream, uploads the NCO tables.  `hip_stream` is a
 * hipStream_t; NULL means HIP's default (null) stream. */
int wr_dev_open(wr_dev **dev, int device_index, void *hip_stream);
int wr_dev_close(wr_dev *dev);
int wr_dev_sync(wr_dev *dev);
void *wr_dev_stream(wr_dev *dev);
/* device memory for callers without another allocator (the C++ host classes) */
int wr_dev_malloc(wr_dev *dev, size_t bytes, void **ptr_dev);
int wr_dev_free(wr_dev *dev, void *ptr_dev);
int wr_dev_upload(wr_dev *dev, void *dst_dev, const void *src_host, size_t bytes);    /* sync */
int wr_dev_download(wr_dev *dev, void *dst_host, const void *src_dev, size_t bytes);
/* For callers that upload the same host buffer block after block (DspSource's output vector,
 * dspblock.h:118, 130-137): page-lock it once, then enqueue the copy and carry on -- the DMA runs
 * beside the caller's own work.  The buffer must not be written until wr_dev_wait_uploads()
 * (or wr_dev_sync) returns, and must be unregistered before it is freed.
 * Register memory that OWNS its pages -- a mapping of its own, as the allocator gives any large vector; page-aligned with
 * its last page to itself if it is carved out of something larger.  A registered range that shares a page with other
 * allocations, or whose address the allocator hands out again, can collide with the page locks the HIP runtime takes on
 * the fly for copies into pageable memory: on ROCm 7.2 that aborts the process (profiles/r04_abort_hunt.txt). */
int wr_dev_host_register(wr_dev *dev, void *host, size_t bytes);
int wr_dev_host_unregister(wr_dev *dev, void *host);
int wr_dev_upload_async(wr_dev *dev, void *dst_dev, const void *src_host, size_t bytes);
int wr_dev_wait_uploads(wr_dev *dev);  /* sync */
/* The same, leaving the `newest` (0..3) most recent uploads in flight: for a source that alternates between two (or more)
 * buffers -- it may refill buffer A as soon as everything but the upload out of buffer B has completed, and the host
 * then runs a block ahead of the GPU instead of in step with it. */
int wr_dev_wait_uploads_but(wr_dev *dev, unsigned int newest);
/* wr_dev_upload_async on the library's own upload stream: the copy runs beside what the device's stream is doing, and the
 * device's stream waits for it, so work enqueued after the call sees `dst_dev` filled.  A caller that ALTERNATES between two
 * `dst_dev` buffers gets the transfer of block b + 1 beside the kernels of block b: the copy waits only for the work that was
 * enqueued before the call after the last one that wrote the same `dst_dev` (rule for the caller: once the next block has been
 * uploaded into the other buffer, enqueue no more readers of this one).  `src_host` page-locked (wr_dev_host_register) for
 * the copy to be a DMA nobody waits for; counts as an upload in flight like wr_dev_upload_async. */
int wr_dev_upload_ahead(wr_dev *dev, void *dst_dev, const void *src_host, size_t bytes);

/* ------------------------------------------- one kernel per reference block -- */
/* DownConverter::process (dsp/downconverter.cxx:91-114).  Frame n uses phase
 * (*phase_io + n*phase_step) mod 2^31; on return *phase_io is the phase after the
 * block (the member DownConverter::phase).  Bit-identical to the reference. */
int wr_mix(wr_dev *dev, const float *in_dev, float *out_dev, size_t nframes,
           unsigned int *phase_io, int phase_step);

/* LowPass::process (dsp/lowpass.cxx:131-162) for `channels` interleaved channels.
 * history_dev holds (63*channels) floats: the last 63 input frames of the previous
 * call (zeros at start, lowpass.cxx:138-139); it is updated in place.
 * out_dev receives (nframes/decimation)*channels floats.  Bit-identical. */
int wr_fir_decimate(wr_dev *dev, const float *in_dev, size_t nframes, unsigned int channels,
                    unsigned int decimation, const float *coeff_host /* [64] */,
                    float *history_dev, float *out_dev);
/* the same for fir_length taps: history_dev holds (fir_length-1)*channels floats */
int wr_fir_decimate_n(wr_dev *dev, const float *in_dev, size_t nframes, unsigned int channels,
                      unsigned int decimation, unsigned int fir_length, const float *coeff_host /* [fir_length] */,
                      float *history_dev, float *out_dev);
/* how many stand-alone block kernels (wr_mix, wr_fir_decimate(_n), wr_demod) this process has run so far: 0 while every
 * Receiver rides a tuner batch */
unsigned long long wr_block_kernel_calls(void);

/* Demodulator::process (dsp/demodulator.cxx:77-115).  prev_io[2] = {prev_i,prev_q}
 * (host), updated on return. */
int wr_demod(wr_dev *dev, int mode, const float *in_dev, size_t nframes,
             float *prev_io /* [2] host */, float *out_dev);

/* The level of a plain block of IQ frames iq_dev[nframes][2] (a stand-alone Demodulator's input): *mean_host = the mean
 * and *peak_host = the largest of e = i*i + q*q over the block, linear powers with full scale 1.0 (either may be NULL).
 * wr_tuner_chan_levels' kernels on one column, so the same rule of summation and the same bits for the same frames.
 * Synchronous; counted by wr_block_kernel_calls.  WR_ERR_ARG: NULL dev or iq_dev, nframes == 0. */
int wr_iq_levels(wr_dev *dev, const float *iq_dev, size_t nframes, float *mean_host, float *peak_host);

/* RTL-SDR byte format to float, (u8 - 128)/128 (io/rtlsdrtuner.cxx:106) */
int wr_u8_to_f32(wr_dev *dev, const uint8_t *in_dev, float *out_dev, size_t count);
/* the same straight out of HOST memory page-locked with wr_dev_host_register -- a quarter of the float block's
 * bytes over PCIe.  Counts as an upload in flight: the host buffer must not be rewritten until wr_dev_wait_uploads
 * (or wr_dev_sync; wr_dev_wait_uploads_but for a source that alternates between buffers).
 * The bytes cross PCIe as a DMA copy on a stream of the library's own (into one of two internal raw buffers in turn), the
 * device's stream waits for the copy and converts: work enqueued after the call sees `out_dev` filled, in stream order
 * like any kernel's output, and the transfer of block b + 1 runs beside the kernels of block b. */
int wr_u8_to_f32_from_host(wr_dev *dev, const uint8_t *in_host_registered, float *out_dev, size_t count);
/* r04, sparse staging: of a block of `nframes` IQ frames in page-locked host memory (bytes when is_u8, else float32
 * pairs) bring over only what a tuner whose channel filters all have `length` taps and decimate by `period` reads --
 * frames [k * period - (length - 1), k * period] of every output frame k (dsp/lowpass.cxx:145-159), widened to 16-byte
 * boundaries -- plus the last `tail_frames` frames (the next block's filter history; a SpectrumSink's current frame), to
 * the SAME positions of the float block at `out_dev`; the frames in between are left as they are.  At BASELINE config 2
 * (length 64, period 400) that is a sixth of the block over PCIe.  The kernel reads the host memory itself, on the device's
 * stream (in order with the tuner's launches behind it); counts as an upload in flight like the call above.
 * Windows of any length up to 4096 frames (a window longer than a wave takes rounds).
 * A submit that follows must use the same `length` and `period` for ALL its receivers. */
int wr_stage_windows_from_host(wr_dev *dev, const void *in_host_registered, int is_u8, float *out_dev, size_t nframes,
                               unsigned int period, unsigned int length, size_t tail_frames);

/* ------------------------------------------------- fused per-tuner path -- */
/* One wr_tuner = one FrontEnd's tuner (radio.cxx:120-133) with all the Receivers
 * attached to it (radio.cxx:151-156).  Every receiver chain
 * DownConverter -> LowPass -> Demodulator -> LowPass (radio.cxx:68-82) of the tuner
 * is evaluated by ONE launch sequence per input block.
 * max_block_frames bounds nframes of wr_tuner_submit; max_channels <= WR_MAX_CHANNELS
 * (WR_ERR_ARG otherwise; the reference has no limit but its CPU, radio.cxx:151-156). */
#define WR_MAX_CHANNELS 4096
int wr_tuner_create(wr_tuner **tuner, wr_dev *dev, unsigned int input_rate,
                    unsigned int max_channels, size_t max_block_frames, int nco_mode);
int wr_tuner_destroy(wr_tuner *tuner);

/* Receiver() + FrontEnd::addReceiver (radio.cxx:62-90,151-156).  The new channel
 * starts with phase 0, zero histories, prev_i = prev_q = 0, IF 0, AM, and no
 * filters: it must be given both filters before the next submit. */
int wr_chan_add(wr_tuner *tuner, int *chan);
int wr_chan_remove(wr_tuner *tuner, int chan);
int wr_chan_count(wr_tuner *tuner, int *count);

/* Setters are STAGED and take effect at the next wr_tuner_submit (the reference
 * applies them mid-block from other threads without locking). */
/* DownConverter::setIF (dsp/downconverter.cxx:59-67) */
int wr_chan_set_if(wr_tuner *tuner, int chan, int if_hz);
/* LowPass::setPassband + setOutputSampleRate + init (dsp/lowpass.cxx:55-61,72-79,
 * 81-116).  stage 0 = channel filter (input = tuner rate, 2 ch), stage 1 = audio
 * filter (input = channel rate, 1 ch).  out_rate must divide the stage's input
 * rate (WR_ERR_RATE otherwise, dspblock.cxx:126-130).  Changing out_rate resets
 * the histories of the channel (as stop()/start() does, lowpass.cxx:118-129). */
int wr_chan_set_filter(wr_tuner *tuner, int chan, int stage, unsigned int passband,
                       unsigned int out_rate);
/* same with caller-designed taps */
int wr_chan_set_taps(wr_tuner *tuner, int chan, int stage, const float *coeff_host /* [64] */,
                     unsigned int decimation);
/* LowPass::_firLength as a run-time value (dsp/lowpass.cxx:38-39 FIXME, :102-110, :167-189 are
 * written in terms of it) INSIDE the fused path: fir_length a power of two in [2, 64].  A shorter
 * filter is the 64-tap filter with its oldest taps zero, bit for bit (the sum runs oldest sample
 * first, lowpass.cxx:150-158).  The CHANNEL filter (stage 0) may also have 128 or 256 taps
 * (WR_FIR_FUSED_MAX): receivers with such a filter form rate groups of their own, which keep the last L - 1
 * MIXED frames per channel as LowPass::block does (lowpass.cxx:138-142).  WR_NCO_EXACT: the reference's own
 * arithmetic -- table lookups, unfused products, oldest sample first -- bit-identical to the reference chain, at
 * the exact kernels' pace.  The other nco modes: the window as L / 64 segments of the ROTATE recurrence, within its
 * tolerance (1e-6), about L / 64 times the 64-tap kernel's time (lane groups whose channels do not share one filter:
 * the reference's arithmetic).  Never a full-rate mixer output.
 * r05: the AUDIO filter (stage 1) and the SECOND channel stage (stage 2) take 128 or 256 taps as well -- rate groups
 * keyed by those lengths too, 127 / 255 rows of history, k_tuner_demod + k_tuner_audio and k_tuner_iq2 with the
 * reference's order of additions: bit-identical to the reference chain in WR_NCO_EXACT, and in every mode as exact as
 * the channel IQ they are fed.  Longer filters (up to WR_FIR_MAX): wr_fir_decimate_n, block by block. */
int wr_chan_set_filter_n(wr_tuner *tuner, int chan, int stage, unsigned int fir_length,
                         unsigned int passband, unsigned int out_rate);
int wr_chan_set_taps_n(wr_tuner *tuner, int chan, int stage, const float *coeff_host /* [fir_length] */,
                       unsigned int fir_length, unsigned int decimation);
/* stage 2 (WR_FILTER_CHANNEL2): an optional SECOND channel LowPass between the first one and the
 * Demodulator -- several LowPass blocks in a row, which is how the reference's own means cut a
 * narrow channel out of a fast stream (one 64-tap stage gives bin 0 below fs / 128,
 * lowpass.cxx:167) -- evaluated inside the tuner's launch sequence.  Its input rate is stage 0's
 * output rate; set it after stage 0 and before stage 1 (the audio filter follows the last channel
 * stage).  WR_STAGE_CHAN_IQ then is ITS output: what the demodulator sees. */
#define WR_FILTER_CHANNEL  0
#define WR_FILTER_AUDIO    1
#define WR_FILTER_CHANNEL2 2
/* The two receiver controls the reference's REST interface names but never implements (af_gain and
 * squelch_threshold are reported as 0 with a FIXME, web/receiverhandler.cxx:112,118-119,127):
 *   af_gain   the audio sample times 10^(dB/20), in float, after the audio filter;
 *   squelch   an audio frame is muted (0.0f) when the mean power i^2 + q^2 of the decimation-many
 *             demodulator input frames behind it is below 10^(dBFS/10); enable = 0 opens it.
 * 0 dB and an open squelch leave every bit as it was. */
int wr_chan_set_af_gain(wr_tuner *tuner, int chan, float gain_db);
int wr_chan_set_squelch(wr_tuner *tuner, int chan, float threshold_dbfs, int enable);
/* Demodulator::setMode (dsp/demodulator.h:49) */
int wr_chan_set_mode(wr_tuner *tuner, int chan, int mode);
/* ask for WR_STAGE_CHAN_IQ / WR_STAGE_DEMOD to be kept for wr_chan_fetch (audio
 * always is).  A bitmask of (1 << stage). */
int wr_tuner_keep_stages(wr_tuner *tuner, unsigned int stage_mask);

/* streaming state of one channel: DownConverter::phase (downconverter.h:58),
 * Demodulator::prev_i/q (demodulator.h:60-61).  (The reference never sets the phase from
 * outside; under WR_NCO_ROTATE doing so also empties the channel filter's history, because
 * that mode keeps the NCO's turn into the next frame rather than its value.) */
int wr_chan_get_state(wr_tuner *tuner, int chan, unsigned int *phase, float *prev_iq /* [2] */);
int wr_chan_set_state(wr_tuner *tuner, int chan, unsigned int phase, const float *prev_iq);

/* DspSource::run for this tuner (dsp/dspblock.h:134, radio.cxx:56-59): push one
 * block of `nframes` IQ frames through every channel.  where = WR_HOST: iq is host
 * memory, copied to the device first; WR_DEVICE: iq is already in HBM and is read
 * in place (it must stay valid until the stream has passed this call). Async.
 * r04: a WR_HOST block in PAGE-LOCKED memory (wr_dev_host_register, hipHostMalloc) whose receivers all decimate alike
 * by at least twice their channel filter's length is staged sparsely -- only the frames under the taps and the block's
 * tail cross PCIe, read by a kernel on the device's stream (see wr_stage_windows_from_host); like any copy out of
 * page-locked memory it is asynchronous: the block must stay untouched until wr_dev_wait_uploads / wr_dev_sync.
 * wr_tuner_last_staging says how the last WR_HOST block travelled:
 * 0 none yet, 1 copied whole, 2 staged sparsely, 3 (r06) streamed: a wr_tuner_submit_u8 block out of page-locked memory
 * under wr_tuner_set_streaming(tuner, 2) -- its bytes cross PCIe as a DMA copy on the library's upload stream and the
 * streaming launch's doorbell is rung by a stream memory operation behind them; nothing waits, and the block must stay
 * untouched until wr_dev_wait_uploads (as for any asynchronous upload).  wr_tuner_stream_host_blocks counts them.  The
 * WHOLE block crosses the link that way (sparse staging brings over a sixth at BASELINE config 2), and whatever else the
 * caller queues on the upload stream in front of a block (wr_dev_upload_ahead, wr_u8_to_f32_from_host) holds its doorbell
 * up: copies of 16 KB or less are copy kernels on this runtime and do not start beside an open launch -- for the same reason a
 * block of 16 KB or less (8192 frames) is not streamed this way: it goes the ordinary way. */
int wr_tuner_last_staging(wr_tuner *tuner, int *how);
int wr_tuner_submit(wr_tuner *tuner, const float *iq, size_t nframes, int where);
/* the same for a block in the RTL-SDR byte format (unsigned 8-bit interleaved IQ, what
 * RtlSdrTuner::dataReady receives, io/rtlsdrtuner.cxx:86-117): the (u8 - 128)/128
 * conversion of rtlsdrtuner.cxx:106 happens in the kernel's load stage, so a quarter of
 * the bytes cross PCIe and leave HBM.  Results are identical to converting first. */
int wr_tuner_submit_u8(wr_tuner *tuner, const uint8_t *iq_u8, size_t nframes, int where);

/* The demodulator + audio filter of a block (its "post stage") need not run inside the submit
 * that brought the block: where the kernel variant allows (WR_NCO_ROTATE, one channel filter per
 * lane group, audio decimation 1..6, demodulator output not kept) it is launched together with
 * the NEXT block's down-conversion, in the same kernel, so that a continuous stream costs one
 * launch per block.  Every call that reads results (wr_chan_fetch, wr_tuner_fetch_audio_all,
 * wr_tuner_audio_dev, wr_chan_get_state) or changes channel parameters launches a pending post
 * stage first, so nothing is ever observed out of order; wr_tuner_flush does only that (e.g. at
 * the end of a stream consumed through the audio ring).  WR_DEFER_POST=0 in the environment
 * turns the deferral off. */
int wr_tuner_flush(wr_tuner *tuner);

/* results of the last submit.  Frames per channel: CHAN_IQ nframes/d1 (x2 floats),
 * DEMOD nframes/d1, AUDIO nframes/d1/d2 -- the truncating arithmetic of
 * dspblock.cxx:177-178.  Synchronises the stream. */
int wr_chan_fetch(wr_tuner *tuner, int chan, int stage, float *out_host, size_t out_capacity,
                  size_t *count);
/* all channels' audio of the last submit, still on the device: audio of channel
 * slot s starts at (*audio_dev) + s * (*chan_stride); slot = wr_chan_slot(). */
int wr_tuner_audio_dev(wr_tuner *tuner, const float **audio_dev, size_t *chan_stride,
                       size_t *frames);
int wr_chan_slot(wr_tuner *tuner, int chan, int *slot);
/* every channel's audio of the last submit in ONE device-to-host copy (what the 256
 * AudioStreamManager sinks of a tuner consume, web/audiostream.cxx:65-73): channel slot s
 * lands at out_host + s * (*chan_stride); *slots_used rows are copied.  Synchronises. */
int wr_tuner_fetch_audio_all(wr_tuner *tuner, float *out_host, size_t out_capacity,
                             size_t *chan_stride, size_t *frames, unsigned int *slots_used);
/* ---- audio sink boundary: a ring of pinned host buffers ----
 * With a ring of `depth` >= 1 slots, ONE asynchronous device-to-host copy of all channels' audio
 * is queued into the next free slot right behind the kernel that produces it (with a deferred
 * post stage, see wr_tuner_flush: behind the next submit's launch, or behind the flush), and
 * nothing waits: the consumer side (the 256
 * AudioStreamManager sinks of a tuner, web/audiostream.cxx:65-73, or a recorder) takes the
 * blocks in order with acquire/release, typically from another thread or one block later,
 * so that the copy and the consumers overlap the next block's kernels.  Like the reference's
 * tuner ring (io/rtlsdrtuner.cxx:100-117) a full ring drops the NEW block's audio and counts
 * an overrun.  Blocks submitted while the tuner's channels do not all share one pair of
 * decimations are not queued (fetch per channel then).  depth 0 frees the ring.
 * r04: a deferred post stage writes its audio into the slot ITSELF (the slot is page-locked host memory mapped into the
 * device's address space; the kernel stores every sample there as well as in device memory), so the block is in the ring
 * when its launch has run and no copy is enqueued behind it. */
int wr_tuner_audio_ring(wr_tuner *tuner, unsigned int depth);
/* oldest block not yet released: waits for its copy, then channel slot s (wr_chan_slot) is at
 * (*audio_host) + s * (*chan_stride), *frames floats each; *seq counts submits from 0 (gaps =
 * overruns).  WR_ERR_STATE when nothing is queued.  The slot stays valid until released. */
int wr_tuner_audio_ring_acquire(wr_tuner *tuner, const float **audio_host, size_t *chan_stride,
                                size_t *frames, unsigned int *slots_used, unsigned long long *seq);
int wr_tuner_audio_ring_release(wr_tuner *tuner);
/* *ready = 1 when the oldest queued block's copy has landed: acquire would return without waiting */
int wr_tuner_audio_ring_ready(wr_tuner *tuner, int *ready);
int wr_tuner_audio_ring_stats(wr_tuner *tuner, unsigned int *queued, unsigned long long *overruns);
/* the number the NEXT wr_tuner_submit* of this tuner will carry (the `seq` of its ring entry): submits numbered so far,
 * whether or not they went through -- a caller that matches ring entries to its own blocks asks here instead of
 * keeping a count of its own beside the library's.  From the thread that submits. */
int wr_tuner_submit_count(wr_tuner *tuner, unsigned long long *submits);
/* LowPass::deinit + init (dsp/lowpass.cxx:118-129, 81-116): both filter histories of the
 * channel become empty again; NCO phase and Demodulator prev_i/q are kept (quirk Q5). */
int wr_chan_reset_history(wr_tuner *tuner, int chan);
/* Time sharding of ONE stream over several GPUs (BASELINE config 5; the reference has no
 * counterpart, its pipeline is one thread, radio.cxx:56-59): put every channel of the tuner in
 * the state it has when the stream STARTS at `frame` -- filter histories empty
 * (lowpass.cxx:138-139), Demodulator::prev_i/q zero (demodulator.cxx:60-70) -- except
 * DownConverter::phase, which takes its closed-form value after `frame` input frames from
 * phase 0 (downconverter.cxx:103).  A block [halo | chunk] submitted next reproduces the
 * sequential result for the chunk once the first halo/(D1*D2) audio frames are dropped
 * (webradio_amd/timeshard.py).  One call, no per-channel traffic -- and no launch: the next submit's launch
 * computes the phase itself and reads all-zero state sets, and a block's demodulator + audio filter that are
 * still waiting for that submit ride in it as usual (one launch per chunk).  Whatever else touches the tuner's
 * state in between (a getter, a setter, a kept demodulator stage, a second or a long channel-filter stage)
 * makes the seek real first. */
int wr_tuner_seek(wr_tuner *tuner, unsigned long long frame);
/* The halo ring of such a time-sharded stream (chunk c on rank c mod world, the halo of
 * every chunk -- the last H frames of the one before it, webradio_amd/timeshard.py: halo_frames --
 * from the ring neighbour).  What a LowPass carries from block to block in a member
 * (dsp/lowpass.cxx:133-142) here crosses GPUs: ONE ncclSend / ncclRecv pair per chunk in one group,
 * rank r -> r + 1, on RCCL directly (librccl.so.1 is looked up when the first wr_ring_* call
 * needs it; WR_ERR_NODEV if it is not there -- nothing else in the library depends on it).
 *   wr_ring_make_id   rank 0 makes the 128-byte rendezvous id (ncclGetUniqueId); the host gets the
 *                     bytes to the other ranks by its own means (a file, MPI, torch.distributed)
 *   wr_ring_create    every rank, collectively (ncclCommInitRank); one process per GPU
 *   wr_ring_exchange  enqueue one pair on the ring's own stream: send `nfloats` floats at send_dev
 *                     to rank + 1, receive as many from rank - 1 into recv_dev.  It is ordered
 *                     after everything the device's stream (wr_dev_open) holds at this moment and
 *                     returns at once -- issue it a round ahead: the halo is input, not a result
 *   wr_ring_wait      the device's stream waits (event to event, no host wait) for the last
 *                     exchange; then submit [halo | chunk] as usual
 * At world = 1 the neighbour is the rank itself (a device copy through RCCL). */
int wr_ring_id_bytes(void);
int wr_ring_version(int *version);                 /* ncclGetVersion of the RCCL that was loaded */
int wr_ring_make_id(void *id_host, size_t nbytes);
int wr_ring_create(wr_ring **ring, wr_dev *dev, const void *id_host, size_t nbytes, int rank, int world);
int wr_ring_exchange(wr_ring *ring, const float *send_dev, float *recv_dev, size_t nfloats);
/* The same, ordered behind the TUNER's launches so far instead of behind everything the device's stream holds: for a
 * halo that is input (already in device memory) received into a buffer only the tuner reads.  Needs
 * wr_tuner_mark_launches(tuner, 1): every launch that reads a submitted block then stamps an event with its own
 * completion signal, and the exchange waits for that -- nothing is put on the device's stream (an event record there
 * sits between two launches: 11 us a chunk).  The rule for the caller: `send_dev` is complete when the call is made,
 * `recv_dev` has no reader other than blocks already submitted to `tuner`.  Blocks the tuner still holds
 * (wr_tuner_set_blocks_per_launch) are launched by the call; blocks launched before marking was switched on are covered
 * by one record made when it is switched on; a tuner that does not mark its launches is WR_ERR_STATE. */
int wr_tuner_mark_launches(wr_tuner *tuner, int enable);
int wr_ring_exchange_after(wr_ring *ring, wr_tuner *tuner, const float *send_dev, float *recv_dev, size_t nfloats);
int wr_ring_wait(wr_ring *ring);
int wr_ring_info(wr_ring *ring, int *rank, int *world, unsigned long long *exchanges);
int wr_ring_destroy(wr_ring *ring);
/* scale applied to the audio as it is stored (default 1).  The MP3 encoder behind every
 * Receiver multiplies by 32768 before LAME (web/mp3encoder.cxx:65-72); a sink that wants
 * that format gets it from the audio kernel's store instead of a host loop. */
int wr_tuner_set_audio_scale(wr_tuner *tuner, float scale);

/* For callers whose blocks already sit in device memory (a resident recording, a capture ring):
 * up to `nblocks` consecutive WR_DEVICE submits whose buffers lie back to back, are equally long
 * and hold whole audio frames are HELD -- pointer and length, the caller keeps the memory alive --
 * and go out as ONE launch over the joined block when the last one arrives, when a submit does
 * not follow on, or when anything reads results or changes parameters (wr_tuner_flush, every
 * fetch and getter, every setter -- which so still takes effect at the boundary after the last
 * block submitted).  The outputs are the same bits (a frame does not
 * depend on where the stream is cut, DspBlock::run's only block-size effect being the truncation
 * of dspblock.cxx:177-178, which whole audio frames avoid); what changes is that they arrive per
 * group: the audio array, wr_chan_fetch and a ring entry then cover all blocks of the group, and
 * the tuner must have been created with max_block_frames >= nblocks * block.  The fixed costs of a
 * launch (start-up, the waves that finish early) are paid once per group: 32.8 -> 30.0 us per block
 * at BASELINE config 2 with nblocks = 4.  1 (the default) = off. */
int wr_tuner_set_blocks_per_launch(wr_tuner *tuner, unsigned int nblocks);

/* r05 -- the streaming launch.  The reference hands a block's output on within the run() that brought the block
 * (dsp/dspblock.cxx:169-212) and its tuner thread swaps the next block in whenever it has one
 * (io/rtlsdrtuner.cxx:265-285).  With `enable` != 0 the WR_DEVICE blocks of a tuner stop costing a kernel launch each:
 * the first opens ONE persistent launch, every following block of the same size and format rings its doorbell (a
 * descriptor and a counter in page-locked host memory -- wr_tuner_submit then returns after two stores), and the
 * launch takes the block up where it stands.  A block's demodulator and audio filter start the moment its last
 * channel-rate frame is out, whether or not another block follows, and its audio ring entry (wr_tuner_audio_ring)
 * becomes ready then -- no wr_tuner_flush needed, the launch stays open.  Everything else that touches the tuner (a
 * setter, a getter, wr_tuner_flush, a block of another size or out of host memory, a wait for the device's stream
 * through this library) closes the launch first: it finishes the blocks it was given and ends.  The results are the same
 * bits as with one launch per block.
 *   Taken up by: WR_NCO_ROTATE tuners with one rate group, at most 1024 channels with 64-tap channel filters, at most 4
 * distinct ones in every lane group of 64 channel slots (a passband per receiver streams as long as no lane group mixes
 * more than 4; a channel-filter setter closes the launch like any setter, and the next block opens another if the new
 * filters still qualify), no second channel stage, an audio decimation of 1..6, 8 or 10, an audio filter of 64 or 128 taps
 * (wr_chan_set_filter_n) or of 256 taps with an audio decimation of 1..3 (beyond it the launch has no room for its window:
 * a launch per block, as before), blocks of whole audio frames that hold at least as many channel-rate frames as the audio
 * filter has taps, no kept demodulator rows
 * (wr_tuner_keep_stages), no launch marks.  Any other submit goes the ordinary way, silently: wr_tuner_stream_info
 * tells which happened.
 *   Rules for the caller: a block's memory stays untouched until the NEXT block's audio is complete (or the launch is
 * closed and the stream waited for); before waiting for the device's stream by other means than this library
 * (hipStreamSynchronize on a stream handed to wr_dev_open, torch.cuda.synchronize()) call wr_tuner_flush -- an open
 * launch that nobody rings ends by itself only after half a second.  An open launch holds nearly every wave slot and
 * register of the GPU: calls on the same wr_dev close it first (a second tuner of the device that streams too takes
 * turns with it, a launch per block), but work sent to the GPU by other means -- another wr_dev, another process --
 * waits until the launch has ended; one streaming launch per GPU and process, a second context's tuner goes the
 * ordinary way meanwhile. */
#define WR_STREAM_MAX_BLOCKS 512u   /* blocks ONE streaming launch takes; the submit after them opens the next launch */
/* enable = 2 (r06): byte-format blocks out of page-locked HOST memory stream as well (wr_tuner_submit_u8(..., WR_HOST), see
 * wr_tuner_last_staging) */
int wr_tuner_set_streaming(wr_tuner *tuner, int enable);
/* `live`: a streaming launch is open right now; `launches`, `blocks`: opened / taken so far (any may be NULL) */
int wr_tuner_stream_info(wr_tuner *tuner, int *live, unsigned long long *launches, unsigned long long *blocks);
/* r06: of those blocks, how many came out of page-locked HOST memory (wr_tuner_submit_u8(..., WR_HOST), see wr_tuner_last_staging) */
int wr_tuner_stream_host_blocks(wr_tuner *tuner, unsigned long long *blocks);
/* r06: of the blocks of launches that are over and looked at (any fetch or sync after the close), how many had their demodulator + audio
 * filter run in LONG runs of tiles: the launch cuts a block's post stage into fewer, longer tasks when two further blocks are rung
 * already -- the host is ahead, the launch runs at the package's power limit and longer runs demodulate and read fewer rows twice --
 * and into short ones when the stream is host-paced or ends (a block's audio is out sooner).  Same bits either way. */
int wr_tuner_stream_long_blocks(wr_tuner *tuner, unsigned long long *blocks);

/* Profiling hook, the analogue of the reference's per-block profiler
 * (DspBlock::nsPerFrameOne, dsp/dspblock.h:69-75), with HIP events on the tuner's stream.
 * `enable` = 1: every submit's dominant launch (the fused mixer + channel filter) stamps its
 * own start and stop.  `enable` = n > 1: one event before the launch of every n-th submit and one
 * after the launch n - 1 submits later -- the mean per launch then includes the gaps between
 * launches and costs 1/n of the events' own few microseconds.  wr_tuner_profile_read
 * synchronises, returns the number of launches covered since the last read and their mean
 * duration in milliseconds, and resets the counters. */
int wr_tuner_profile(wr_tuner *tuner, int enable);
int wr_tuner_profile_read(wr_tuner *tuner, unsigned int *launches, double *mean_ms);

/* -------------------------------------------------------- SpectrumSink -- */
/* SpectrumSink::init (io/spectrumsink.cxx:60-77).  fft_size: power of two
 * (spectrumsink.cxx:53-56), 8 <= fft_size <= 1048576.  hop: frames between
 * successive transforms; 0 or fft_size = the reference's back-to-back frames
 * (spectrumsink.cxx:101-121); fft_size/2 = 50 % overlap (BASELINE config 3). */
int wr_spectrum_create(wr_spectrum **spec, wr_dev *dev, unsigned int fft_size, unsigned int hop);
/* The same sink for REAL samples, one float per frame: a receiver's audio, a Demodulator's output.  The reference leaves
 * this open (io/spectrumsink.cxx:62-64: "Check number of channels, select appropriate plan", "Handle real->complex for
 * spectrum of real signals"; :93-100 expects _channels = 1 to work once the plan is right).  The spectrum is what
 * wr_spectrum_create's sink gives for the frames (x[n], 0): same window, same dB expression, fft_size values, the row
 * symmetric about its middle -- computed as a transform of fft_size / 2 packed points and an untangle step, so half the
 * input bytes and half the butterflies.  Every call below that counts frames counts samples on such a spectrum.
 * A real spectrum is never kept aside beside an open streaming launch: a WR_DEVICE push closes the launch like any other
 * call on the device. */
int wr_spectrum_create_real(wr_spectrum **spec, wr_dev *dev, unsigned int fft_size, unsigned int hop);
/* floats per frame: 2 (wr_spectrum_create) or 1 (wr_spectrum_create_real) */
int wr_spectrum_channels(wr_spectrum *spec, unsigned int *channels);
int wr_spectrum_destroy(wr_spectrum *spec);
/* SpectrumSink::process (io/spectrumsink.cxx:88-123): append frames; every time a
 * frame is complete it is windowed and transformed.  Async for WR_DEVICE input.
 *   While a streaming launch is open on the device (wr_tuner_set_streaming) a WR_DEVICE block that holds a whole frame is
 * not transformed then and there -- that would close the launch every block: the newest frame (and what follows it) is
 * copied aside by the DMA engine and transformed when a getter below asks for it; only the most recent frame is
 * observable anyway (spectrumsink.cxx:93-94's FIXME, waterfallhandler.cxx:56-61 polls at 5 Hz).  A poll then costs one
 * closed launch, a block nothing.  wr_spectrum_lazy_info counts both. */
int wr_spectrum_push(wr_spectrum *spec, const float *iq, size_t nframes, int where);
int wr_spectrum_lazy_info(wr_spectrum *spec, unsigned long long *deferred_pushes, unsigned long long *resolves);
/* SpectrumSink::getSpectrum (io/spectrumsink.cxx:125-142): dB, fft-shifted, of the
 * most recent transform.  WR_ERR_STATE before the first complete frame (the
 * reference returns uninitialised memory there, quirk Q8). */
int wr_spectrum_get_db(wr_spectrum *spec, float *magnitudes_host /* [fft_size] */);
/* raw complex bins of the most recent transform (FFTW order), for tests */
int wr_spectrum_get_bins(wr_spectrum *spec, float *bins_host /* [2*fft_size] */);
int wr_spectrum_frames_done(wr_spectrum *spec, unsigned long *frames);
/* One waterfall row as the browser draws it (web/waterfallhandler.cxx:56-69 +
 * html/waterfall.js:92-109), computed on the device from the most recent transform:
 *   db_row_host[width]   (optional) dB per pixel column; non-finite values become -10000
 *                        (waterfallhandler.cxx:65-68)
 *   palette_host[width]  (optional) palette index clamp(floor((dB + 50) / 25 * 255), 0, 255)
 * `width` <= fft_size, fft_size % width == 0.  hold = 0: the bin the UI's overdraw leaves
 * visible in each column (the LAST of the fft_size/width bins that map to it);
 * hold = 1: the maximum of those bins (peak hold, loses no narrow carrier). */
int wr_spectrum_get_waterfall_row(wr_spectrum *spec, unsigned int width, int hold,
                                  float *db_row_host, uint8_t *palette_host);
/* transform `nframes_fft` whole frames laid out back to back at a fixed hop in
 * device memory and write dB rows (waterfall): frame f starts at iq_dev + 2*f*hop
 * (a real spectrum: at iq_dev + f*hop).
 * db_dev receives nframes_fft rows of fft_size floats (fft-shifted). Async. */
int wr_spectrum_batch_db(wr_spectrum *spec, const float *iq_dev, size_t nframes_fft,
                         float *db_dev);
/* The same for rows: the first fft_size frames of each of `nrows` rows lying `row_stride` frames apart
 * (row_stride >= fft_size, else WR_ERR_ARG) to nrows dB rows.  With wr_tuner_audio_dev's pointer and chan_stride on a
 * real spectrum: the audio spectrum of every receiver of a block (which needs fft_size audio frames or more) in one
 * launch sequence.  Async; closes an open streaming launch first, like wr_spectrum_batch_db. */
int wr_spectrum_batch_db_rows(wr_spectrum *spec, const float *in_dev, size_t row_stride, size_t nrows,
                              float *db_dev);
/* MEAN and PEAK-HOLD spectra over all frames of a block: what a display that polls at 5 Hz (web/waterfallhandler.cxx:56-61)
 * needs so as not to miss what went by between two polls.  `ngroups` groups of `nframes_fft` frames each: frame f of group
 * g starts g * group_stride + f * hop frames into in_dev (hop: the spectrum's own; a real spectrum: one float per frame).
 * ngroups = 1 (any group_stride) is wr_spectrum_batch_db's layout; hop = fft_size, nframes_fft = 1, ngroups = nrows is
 * wr_spectrum_batch_db_rows'; wr_tuner_audio_dev's pointer with chan_stride as group_stride, on a real spectrum, gives the
 * averaged audio spectrum of every receiver of a block.  mean_dev and peak_dev each receive ngroups rows of fft_size floats,
 * fft-shifted as wr_spectrum_get_db shifts; either may be NULL, not both.
 *   The rule, for bin k of a group, (re_f, im_f) being what the transform of frame f gives there:
 *     p_f  = fl(fl(re_f * re_f) + fl(im_f * im_f))                       (no fused multiply-add)
 *     sum  = ((p_0 + p_1) + p_2) + ...      one float accumulator, in frame order
 *     mean = sum / (float)nframes_fft,      peak = the largest p_f
 *   linear != 0: the rows hold mean and peak; else 10 * log10f(x) - 20 * log10f(fft_size), wr_spectrum_get_db's expression.
 * The result does not depend on the launches' grids, on how the call is cut into chunks, or on ngroups.  Non-finite input
 * gives unspecified values in its group's rows and nothing else.
 *   Every size and both kinds of spectrum.  The transforms write bins to a scratch area of the spectrum's own (64 MB at
 * most, freed by wr_spectrum_destroy) and a reduce kernel walks them; longer calls go through it in chunks, over frames
 * and over groups, with the same bits.  Where one workgroup transforms a frame (IQ up to 8192 points, real up to 16384) a
 * chunk is two launches however many groups it holds; on the larger sizes the transform is a loop over the groups.
 *   Async on the device's stream; closes an open streaming launch first, like wr_spectrum_batch_db.  The spectrum's own
 * frames (wr_spectrum_push, frames_done, get_bins, get_db) are left alone.
 *   WR_ERR_ARG: spec or in_dev NULL, both outputs NULL, nframes_fft = 0, ngroups > 1 with group_stride < fft_size.
 * ngroups = 0: WR_OK, nothing written.
 *   Left out on purpose: an averaging mode of the host runtime's SpectrumSink class, which keeps only the newest frame
 * beside a streaming launch; an averaged wr_tuner_chan_spectra, whose kernel works on the column layout of channel IQ;
 * exponential averaging across calls -- a caller blends linear rows. */
int wr_spectrum_batch_avg(wr_spectrum *spec, const float *in_dev, size_t nframes_fft,
                          size_t ngroups, size_t group_stride, int linear,
                          float *mean_dev, float *peak_dev);
/* Waterfall rows on the device: wr_spectrum_get_waterfall_row's reduction and palette (the last bin or, hold = 1, the
 * maximum per pixel column; non-finite becomes -10000; the palette expression in double) on `nrows` fft-shifted dB rows of
 * fft_size floats in device memory -- wr_spectrum_batch_avg's or wr_spectrum_batch_db's.  db_rows_dev[nrows][width] and
 * palette_dev[nrows][width]: either may be NULL, not both.  `width` <= fft_size, fft_size % width == 0, else WR_ERR_ARG.
 * One launch, async: a block goes from samples to pixel rows without visiting the host. */
int wr_spectrum_rows_waterfall(wr_spectrum *spec, const float *db_dev, size_t nrows, unsigned int width, int hold,
                               float *db_rows_dev, uint8_t *palette_dev);

/* BAND SCAN: the noise floor and the occupied segments of spectrum rows, on the device -- where in the band there is
 * something to listen to, as a few records of 24 bytes per row instead of the rows themselves.
 *   Input is `nrows` rows of n = fft_size floats in device memory.  Any rows of that shape are accepted: the fft-shifted dB
 * rows of wr_spectrum_batch_avg, wr_spectrum_batch_db, wr_spectrum_batch_db_rows and wr_tuner_chan_spectra; with `linear`,
 * the power rows of wr_spectrum_batch_avg(linear = 1).
 *   The rule (a wr_detect_rule):
 *     bin0, nbins   the part of each row that is looked at            bin0 + nbins <= n, nbins >= 8
 *     span          bins that share one noise floor                   8 <= span, nbins % span == 0
 *     percent       which order statistic is the floor                0 .. 100
 *     threshold     float, finite
 *     linear        int
 *     max_gap       cold bins a segment bridges                       <= nbins
 *     min_width     narrowest segment that is kept                    1 .. nbins
 * (the window bin0 / nbins exists for one half of a real spectrum's symmetric row, and for leaving out band edges or the DC
 * spike).  Anything outside the limits gives WR_ERR_ARG, with a message that names the call and the field.
 *   Order of floats.  key(x): with u the float's 32 bits, u ^ 0xFFFFFFFF if the sign bit is set, else u | 0x80000000.  Keys
 * order -inf < ... < -0 < +0 < ... < +inf.  NaNs never take part (x != x).
 *   Floor of span j (`span` bins from bin0 + j * span).  Let m be the number of non-NaN values in the span.  The floor is
 * the value whose key is the rank-th smallest, counting from 0, with rank = ((m - 1) * percent) / 100 in integer division.
 * Its bits are an input's bits.  m = 0: the floor is NaN (0x7FC00000) and the span has no hot bin.
 *   Hot bins.  t = fl(floor + threshold), or with `linear` t = fl(floor * threshold): one float32 operation with no fusion.
 * Bin k is hot iff row[k] >= t, which is false when either side is NaN.
 *   Segments.  Take the hot bins h_0 < h_1 < ... of the window.  h_i starts a segment iff i = 0 or
 * h_i - h_{i-1} - 1 > max_gap.  Segments do not wrap round the window's ends and pay no attention to span borders.  A
 * segment has: first and last, its first and last hot bin; hot, the number of its hot bins; peak_bin, the hot bin with the
 * largest key, the lowest index on ties; peak = row[peak_bin]; floor, the floor of the span that holds peak_bin.  A segment
 * is kept iff last - first + 1 >= min_width.
 *   Records.  Bin indices are the row's own, not relative to bin0.  count_dev[r] is the number of kept segments of row r,
 * all of them.  det_dev[r * max_det + i] is the i-th kept segment in ascending `first`, for i < min(count, max_det); entries
 * behind that are not written.  floor_dev[r * (nbins / span) + j] is optional and holds the floors.
 *   Non-finite input has exactly the meaning above and touches nothing but its own row.  Integers decide, apart from the one
 * float operation and the one float compare; the result does not depend on grids or on the number of rows. */
typedef struct {
	unsigned int bin0, nbins;
	unsigned int span;
	unsigned int percent;
	float threshold;
	int linear;
	unsigned int max_gap;
	unsigned int min_width;
} wr_detect_rule;

typedef struct { uint32_t first, last, peak_bin, hot; float peak, floor; } wr_detection;

/* The whole row, span = min(fft_size, 1024), percent = 50 (the median), threshold = 10 (dB above it), linear = 0,
 * max_gap = 1, min_width = 1.  fft_size: a power of two in [8, 1048576], else WR_ERR_ARG.  Needs no device. */
int wr_detect_rule_default(unsigned int fft_size, wr_detect_rule *rule);
/* The frequency of (fractional) bin `bin` of a shifted row: *hz = centre_hz + (bin - fft_size / 2) * sample_rate / fft_size
 * (DC sits at fft_size / 2).  `bin` is a double so that a segment's middle (first + last) / 2 converts too.  WR_ERR_ARG:
 * fft_size no power of two in [8, 1048576], sample_rate = 0, hz NULL.  Needs no device. */
int wr_spectrum_bin_hz(unsigned int fft_size, unsigned int sample_rate, double centre_hz, double bin, double *hz);
/* The rule above on `nrows` rows.  Two launches per chunk of rows: the floors (an exact order statistic by radix select, one
 * workgroup per span and row), then the segments (forward scans with a carry from tile to tile, one workgroup per row -- a
 * 2^20-point row is one workgroup's work).  Both kinds of spectrum, every fft_size, any nrows.  Async on the device's stream;
 * closes an open streaming launch first, like wr_spectrum_rows_waterfall.  max_det = 0 only counts.  Without floor_dev the
 * floors live in the spectrum's own scratch area (wr_spectrum_batch_avg's, freed by wr_spectrum_destroy), 512 KB of it at
 * most: more rows than that holds floors for go through it in chunks of rows, with the same result.
 *   WR_ERR_ARG: spec, rule or count_dev NULL; rows_dev NULL with nrows > 0; det_dev NULL with max_det > 0; a field of the
 * rule outside its limits.  nrows = 0: WR_OK, nothing written.
 *   Left out on purpose: tracking detections from block to block, assigning receivers to them, the integrated power of a
 * segment, detection inside the streaming launch. */
int wr_spectrum_rows_detect(wr_spectrum *spec, const float *rows_dev, size_t nrows, const wr_detect_rule *rule,
                            unsigned int max_det, wr_detection *det_dev, unsigned int *count_dev, float *floor_dev);

/* The CHANNEL spectrum of every receiver of a tuner (a SpectrumSink connected to each Receiver's channel filter,
 * io/spectrumsink.cxx:88-142 behind radio.cxx:68-76): for each channel slot the dB row (fft-shifted, wr_spectrum_get_db's
 * expression) of channel-rate frames [first_frame, first_frame + fft_size) of WR_STAGE_CHAN_IQ of the last submit, in one
 * launch.  Row of slot s (wr_chan_slot) at db_dev + s * fft_size; *slots (optional) = rows written (the group's slots in
 * use, in whole lane groups of 64 as wr_tuner_fetch_audio_all counts them: at most max_channels rounded up to 64, and
 * db_dev needs room for that many rows; rows of slots that hold no channel carry no meaning).
 * `spec`: an IQ spectrum (wr_spectrum_create) of the tuner's wr_dev with fft_size <= 8192; its window and twiddle tables
 * are used, its own frames (wr_spectrum_push, frames_done, bins) are left alone.  Like every getter it sends held blocks
 * out, launches a pending post stage and closes an open streaming launch.  Async on the device's stream.
 * WR_ERR_ARG: NULL arguments, a real spectrum, fft_size > 8192, first_frame + fft_size beyond the last submit's channel
 * frames, a spectrum of another wr_dev.  WR_ERR_STATE: nothing submitted yet, several rate groups. */
int wr_tuner_chan_spectra(wr_tuner *tuner, wr_spectrum *spec, size_t first_frame, float *db_dev, unsigned int *slots);

/* The SIGNAL LEVEL of every receiver of a tuner (an S-meter beside the squelch_threshold and af_gain the reference's REST
 * interface names, web/receiverhandler.cxx:112,118-119): the level of WR_STAGE_CHAN_IQ of the last submit -- what the
 * demodulator sees (dsp/demodulator.cxx:77-115) -- for every channel slot, from one launch sequence.  With
 * e_m = i*i + q*q of channel frame m (two products and one sum, each rounded to float) and K1 = *frames:
 *   mean_host[s]  = sum / (float)K1, a linear power with full scale 1.0.  THE SUM is taken in one order, whatever the
 *                   device and whatever max_channels: frames oldest first in runs of 16 (r_j = e_16j + e_16j+1 + ...),
 *                   the run sums in order in groups of 16 runs, i.e. 256 frames (c_h = r_16h + r_16h+1 + ...), the group
 *                   sums in order (sum = c_0 + c_1 + ...); the last run and the last group are simply shorter; every
 *                   partial starts from its first term (e is never -0, so starting from 0.0f would give the same bits).
 *                   The same frames give the same bits everywhere, and a float restatement of the rule is bit-identical.
 *   peak_host[s]  = the largest e_m.
 *   muted_host[s] = how many of the *audio_frames audio frames of the block the squelch muted (wr_chan_set_squelch's
 *                   test, the audio path's own expression: the sum from 0.0f of the e of the frame's d2 channel frames,
 *                   oldest first, divided by (float)d2, below the threshold); 0 for an open squelch.  The thresholds are
 *                   the ones the last submit's audio was made with: a wr_chan_set_squelch since then shows once a block
 *                   has been submitted with it (a wr_tuner_seek uploads staged settings too).
 * Each array holds *slots entries (the slots in use in whole lane groups of 64, as wr_tuner_fetch_audio_all and
 * wr_tuner_chan_spectra count them: at most max_channels rounded up to 64); the entry of a channel is wr_chan_slot's,
 * entries of slots that hold no channel carry no meaning.  Any of the three arrays, frames, audio_frames and slots may be
 * NULL; all three arrays NULL is WR_ERR_ARG.  Like every getter it sends held blocks out, launches a pending post stage
 * and closes an open streaming launch; then it copies the few bytes out and waits for them.  It changes nothing the next
 * block depends on.  WR_ERR_STATE: nothing submitted yet, several rate groups. */
int wr_tuner_chan_levels(wr_tuner *tuner, float *mean_host, float *peak_host, unsigned int *muted_host, size_t *frames,
                         size_t *audio_frames, unsigned int *slots);

/* AUTOMATIC GAIN CONTROL of a receiver's audio.  The reference has none: its demodulators hand on sqrt(i^2 + q^2), i + q
 * and i - q at whatever level the antenna delivers (dsp/demodulator.cxx:88-104), and its only "AGC" is the RTL-SDR's RF
 * gain mode, one setting for the whole band (io/tuner.h:56-62).  Here every receiver has a gain of its own.
 *
 * THE RULE is this library's own definition, as the ones of af_gain and squelch are.  v[m] is the receiver's audio-filter
 * output after the squelch gate, m counts audio frames over the stream, and all state is ONE unsigned 32-bit word E:
 *   L[m]   = min(bits(v[m]) & 0x7fffffff, 0x7f7fffff)      bits(): the float's own 32 bits; an inf or a NaN counts as FLT_MAX
 *   E[m]   = max(L[m], E[m-1] - step, floor)               integers, the subtraction does not wrap; E[-1] = floor
 *   env[m] = the float whose bits are E[m]                 (positive, finite, normal)
 *   g[m]   = target / env[m]                               one IEEE float32 division, correctly rounded
 *   out[m] = v[m] * g[m], then * af_gain if it is not 1, then * scale if it is not 1     (separate float32 products)
 * The bit pattern of a positive float is a monotone, piecewise-linear log2: an octave (6.02 dB of amplitude) is 2^23
 * units.  So this is a peak detector with
 *   an instant attack: env[m] >= |v[m]|, i.e. |v * g| <= target up to the two roundings;
 *   a release that is linear in (almost) dB: E falls `step` units per audio frame; inside an octave the bit pattern is
 *     linear in the amplitude, not in its logarithm, so the rate in dB/s wobbles between 0.72 and 1.44 of its nominal value
 *     (fastest at the octave's lower end);
 *   exact integer arithmetic: E has ONE value whatever order it is computed in.  In closed form, with a carry C = E[-1]
 *     and U[j] = L[j] + j * step in 64 bits:  E[m] = max(max_{j<=m} U[j] - m * step, C - (m + 1) * step, floor)  -- a prefix
 *     maximum, which is how the GPU computes it; a restatement by the plain loop is bit-identical.
 * The order in a tuner: audio filter -> squelch -> AGC -> af_gain -> scale (wr_tuner_set_audio_scale).  An AGC that is
 * off leaves every bit as it was.
 * Left out on purpose: attack smoothing and a hang time (a sliding maximum over a window longer than a block needs
 * history rows); a host-side C++ block (af_gain and squelch have none either, and the reference has no class to mirror);
 * AGC under time sharding (the state has unbounded memory: a shard that seeks starts from floor).
 *
 * wr_agc_design: the rule's three numbers, on the host in double; needs no device.
 *   *target     = (float)10^(target_dbfs / 20)
 *   *floor_bits = bits((float)(10^(target_dbfs / 20) / 10^(max_gain_db / 20))): the gain never exceeds max_gain_db, and
 *                 silence is no special case
 *   *step       = llround(decay_db_per_s / (20 log10 2) * 2^23 / audio_rate), at most 2^31 (20 dB/s at 10 kHz: 2787)
 * WR_ERR_ARG: a NaN, target_dbfs outside [-100, 0], decay_db_per_s outside [0, 1e4], max_gain_db outside [0, 120], a
 * floor that would be subnormal, audio_rate 0, a NULL result. */
int wr_agc_design(float target_dbfs, float decay_db_per_s, float max_gain_db, unsigned int audio_rate, float *target,
                  unsigned int *floor_bits, unsigned int *step);
/* The rule on a plain block of audio in device memory, in place: `nrows` rows of `nframes` floats, `row_stride` floats
 * apart, row r with target_host[r], floor_bits_host[r], step_host[r] and the state word state_host[r] -- E[-1] on entry
 * (floor_bits to begin a stream with), the row's last E on return, so consecutive calls continue one stream whatever
 * the lengths.  step_host[r] = 0xffffffff: row r has no AGC and is not touched.  af_gain and scale are 1.  Synchronous;
 * counted by wr_block_kernel_calls.  WR_ERR_ARG: NULL arguments, no rows, row_stride < nframes with several rows, a step
 * above 2^31, floor bits that are no positive normal float, a state above 0x7f7fffff, a target that is not positive and
 * finite. */
int wr_agc_rows(wr_dev *dev, float *audio_dev, size_t row_stride, size_t nrows, size_t nframes,
                const float *target_host, const unsigned int *floor_bits_host, const unsigned int *step_host,
                unsigned int *state_host /* [nrows], in and out */);
/* A receiver's AGC inside the tuner.  Staged like every setter and applied at the next block boundary; `step` is derived
 * for the receiver's audio rate, and again when a filter change alters that rate.  Coming on, wr_chan_reset_history and
 * wr_tuner_seek set the state to floor; new settings while it is on keep the state.  enable = 0 turns it off (the other
 * arguments are then ignored).  The AGC runs as one more kernel behind the post stage of a rate group that has one on,
 * in place on the group's audio: wr_chan_fetch(WR_STAGE_AUDIO), wr_tuner_audio_dev, wr_tuner_fetch_audio_all, the audio
 * ring and wr_spectrum_batch_db_rows on the audio rows see its output; WR_STAGE_DEMOD, WR_STAGE_CHAN_IQ and
 * wr_tuner_chan_levels are what they were.  A receiver WITHOUT AGC in such a group goes through the same float products
 * in the same order as before: its audio is bit-identical to the same tuner with no AGC anywhere.  While any receiver
 * has its AGC on, the tuner's blocks are not held back (wr_tuner_set_blocks_per_launch) and do not go into the
 * streaming launch (wr_tuner_set_streaming): an open launch is closed at the boundary where AGC comes on, and streaming
 * resumes when the last one goes off.  With no AGC on, nothing new runs.
 * WR_ERR_ARG: no such channel, wr_agc_design's limits. */
int wr_chan_set_agc(wr_tuner *tuner, int chan, float target_dbfs, float decay_db_per_s, float max_gain_db, int enable);
/* what the last submit used (*enabled, *target, *floor_bits, *step: the numbers uploaded for it; all 0 before the first
 * block with AGC on) and left (*state: E behind the block's last audio frame).  Any result may be NULL.  Reading the state
 * waits for the tuner's work. */
int wr_chan_get_agc(wr_tuner *tuner, int chan, int *enabled, float *target, unsigned int *floor_bits,
                    unsigned int *step, unsigned int *state);
/* *channels_on: receivers whose AGC the last submit ran; *launches: AGC kernels launched for this tuner so far (one per
 * block and rate group with an AGC on, none otherwise).  Either may be NULL. */
int wr_tuner_agc_info(wr_tuner *tuner, unsigned int *channels_on, unsigned long long *launches);

/* TONE BANK: which sub-audible tone (CTCSS) rides on each receiver's audio -- the basis of tone squelch; the same
 * mechanism answers "is there a 1750 Hz burst" and "which DTMF pair".  The reference has nothing of the kind.  A spectrum
 * cannot stand in for it: neighbouring CTCSS tones are 2.3 Hz apart, which needs 0.25 - 0.5 s of audio -- many tuner
 * blocks, and the spectrum calls look at one.  A bank is up to 64 tone correlators per row that integrate across blocks.
 *
 * THE RULE is this library's own definition, as the ones of af_gain, squelch and AGC are.  A bank has
 *   `ntones` tones, 1 to 64, each an unsigned 32-bit phase step (wr_tone_step);
 *   a window of W audio frames, 16 <= W <= 65536;
 *   `max_rows` rows, 1 to 65535.
 * Every row is an independent audio stream cut into consecutive windows of W frames; the count starts at the row's first
 * pushed frame, or after a reset.  For frame j (0 ... W-1) of a window, with audio value v:
 *   v'   = 0.0f if (bits(v) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else v
 *   w    = min(max(v', -64.0f), 64.0f) * 16777216.0f          exact; |w| <= 2^30
 *   p    = (uint32)(j * step_t)                                wraps mod 2^32
 *   i    = p >> 20                                             12 bits
 *   s    = T12[i],  c = T12[(i + 1024) & 4095]                 T12[i] = wr_sin_table()[16 * i]
 *   I_t += (int64) rint(w * c)      Q_t += (int64) rint(w * s)
 *   qv   = (int64) rint(w)          E  += (qv * qv) >> 14      E is per row, not per tone
 * Each of w * c and w * s is one float32 product rounded once; rint rounds to nearest even, and its result fits an int32.
 * At a window's last frame (I_t, Q_t, E) are latched as the row's result and the row's window count goes up by one; the
 * accumulators then start again from 0.  |I|, |Q| <= 2^46 and E <= 2^62: nothing wraps.
 * Everything is integer sums of per-frame terms, so a window's result has ONE value for any grid, any cut of the stream
 * into pushes and any order of summation (integer atomics would not change it); a restatement in numpy is bit-identical.
 * The share of the window's audio power that sits in tone t, computed by the caller in double:
 *   rho_t = 2 (I_t^2 + Q_t^2) / (W * E * 2^14)
 * about 1 for a pure tone at f_t, about 2 / W per tone for white noise; the rectangular window leaks
 * sinc^2(df * W / rate) of it into a tone df away.
 * Left out on purpose: muting audio by tone (the detector reports, the caller decides); a host-side C++ class (the
 * reference has none to mirror, and af_gain, squelch and AGC have none either); window functions other than the
 * rectangular one; per-receiver tone lists (one list per bank); time sharding.
 *
 * wr_tone_step: *step = llround(hz / audio_rate * 2^32); needs no device.  WR_ERR_ARG unless 0 < hz < audio_rate / 2. */
int wr_tone_step(double hz, unsigned int audio_rate, unsigned int *step);
/* WR_ERR_ARG: ntones outside 1..64, window outside 16..65536, max_rows outside 1..65535, a step of 0 or >= 2^31. */
int wr_tones_create(wr_tones **bank, wr_dev *dev, unsigned int max_rows, const unsigned int *steps_host,
                    unsigned int ntones, unsigned int window);
int wr_tones_destroy(wr_tones *bank);
/* Sets the row's accumulators, fill, window count and latched result to 0: the row begins a new stream.  row < 0: every
 * row.  This is what a caller does after wr_tuner_seek, wr_chan_reset_history or a retune of the receiver in that slot:
 * the bank does not watch the tuner.  Asynchronous on the device's stream. */
int wr_tones_reset(wr_tones *bank, int row);
/* The rule on a plain block of rows in device memory: `nrows` rows of `nframes` floats, `row_stride` floats apart; row r of
 * the call is row r of the bank.  Consecutive calls continue the streams whatever the lengths.  A block may hold no
 * window end, one, or many: with many, only the last complete window is latched and the count rises by all of them.
 * Asynchronous on the device's stream; counted by wr_block_kernel_calls.  WR_ERR_ARG: NULL arguments, nrows > max_rows,
 * row_stride < nframes with several rows. */
int wr_tones_push_rows(wr_tones *bank, const float *audio_dev, size_t row_stride, size_t nrows, size_t nframes);
/* Pushes the last submit's audio rows of every channel slot: WR_STAGE_AUDIO as wr_tuner_audio_dev shows it -- after
 * squelch, AGC, af_gain and scale; row = wr_chan_slot.  Rows are counted as wr_tuner_chan_levels counts them (*slots: whole
 * lane groups of 64); rows of slots that hold no channel carry no meaning.  The slots are counted when the push is made, not
 * when the submit was: a receiver removed in between that sat alone in the top lane group makes the push 64 rows shorter, and
 * a bank that resets the rows a push leaves out (resampler, DCS bank, voice bank; not this one) then resets those.  The same
 * holds for wr_tuner_dcs_push, wr_tuner_resamp_push and wr_tuner_voice_push.  rho does not depend on af_gain and scale:
 * they multiply I, Q and sqrt(E) alike.  Like every getter it sends held blocks out, launches a pending post stage and
 * closes an open streaming launch; it changes nothing the next block depends on.  Asynchronous behind that.
 * WR_ERR_STATE: nothing submitted yet, several rate groups, the same submit pushed twice (the bank remembers the tuner's
 * submit count).  WR_ERR_ARG: max_rows below the slot count, a bank of another device. */
int wr_tuner_tones_push(wr_tuner *tuner, wr_tones *bank, unsigned int *slots);
/* The latched result (iq_host[rows][ntones][2]: I, Q; energy_host[rows]: E), the window count and the frames in the open
 * window of every row; *rows = max_rows.  Any array may be NULL, all four NULL is WR_ERR_ARG.  Waits for the device's
 * stream. */
int wr_tones_read(wr_tones *bank, long long *iq_host /* [rows][ntones][2] */, long long *energy_host,
                  unsigned long long *windows_host, unsigned int *fill_host, unsigned int *rows);

/* DCS BANK: which digital-coded squelch code rides on each receiver's audio -- the other half of tone squelch.  DCS is a
 * 23-bit Golay word sent over and over at 134.4 bit/s as sub-audible NRZ under the voice, bit 0 first.  The reference has
 * nothing of the kind.  A bank is up to 128 code words tried on every row, in both polarities, at every evaluation: a bit
 * slicer and a correlator over words, on the audio rows the tone bank takes.
 *
 * THE RULE is this library's own definition, as the ones of af_gain, squelch, AGC, the tones and the resampler are.
 * Everything is an integer after the first line of CHIP SUMS, so a stream has ONE result whatever the grid, the cut into
 * pushes and the order of additions; a restatement in numpy is bit-identical.
 *
 * CODE WORD.  wr_dcs_word(code, &word) takes `code` in 0 ... 511, the three octal digits.
 *   d = code | 0x800                                            the fixed bits 100 sit above the nine code bits
 *   p = d;  twelve times:  if (p & 1) p ^= 0xC75;  p >>= 1      the parity
 *   word = (p << 12) | d                                        bit 0 is sent first
 * 023 -> 0x763813, 754 -> 0x20f9ec, 412 -> 0x79c90a.  The complement of 023's word is a rotation of 047's (an inverted 023
 * IS a 047); all 512 words have weight 7, 8, 11, 12, 15 or 16.  The bank itself takes any 23-bit words.
 *
 * BIT CLOCK.  wr_dcs_step(audio_rate, &step):
 *   step = (672 * 2^32 + (5 * rate) / 2) / (5 * rate)           integer division: 134.4 Hz in units of 2^-32 bit per frame
 * WR_ERR_ARG for any rate whose step is not in [2^19, 2^28]: between 2 and 1024 frames per chip (an eighth of a bit).
 * A bank has ONE clock, as the resampler has: N, the frames pushed since it was created, reset as a whole or sought; 64-bit,
 * kept on the host.  Frame n of the stream belongs to chip
 *   g(n) = floor(n * step / 2^29)                               eight chips per bit
 * The product can pass 2^64: the host reduces the push's first frame (N0 * step mod 2^29, and its chip index), the kernel
 * adds k * step for frame k < 2^28 of the push.
 *
 * CHIP SUMS.  For audio value v:
 *   v'   = 0.0f if (bits(v) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else v
 *   q    = (int64) rint(min(max(v', -64.0f), 64.0f) * 16777216.0f)          the tone bank's cleaning
 *   C[g(n)] += q
 * A chip whose frames were never pushed is 0; after a reset the same goes for the chips in front of the stream.
 *
 * EVALUATION.  Evaluation e = 1, 2, ... happens once all frames of chip 8 e - 1 are in: after N frames floor(g(N) / 8)
 * evaluations have happened, whatever the pushes were; a push may hold none or several.  Each tries eight timing phases
 * f = 0 ... 7:
 *   B_b  = sum_{c < 8} C[8 e - 184 - f + 8 b + c]               b = 0 ... 22
 *   w_f  = sum_b 2^b * [2 * B_b > max_b B + min_b B]            the midpoint of the extremes is the slicer's threshold: it
 *                                                               removes the discriminator's DC whatever the word's weight
 * For code word k of the bank and its 23 rotations rot_r, agreeing bits in both polarities:
 *   agree[k][0] = max_{f, r} (23 - popcount(w_f ^ rot_r(word_k)))
 *   agree[k][1] = max_{f, r} popcount(w_f ^ rot_r(word_k))                  the inverted polarity
 * A polarity matches when agree >= 23 - max_errors.  A match does hits[k][pol] += 1 and run[k][pol] += 1; a miss sets
 * run[k][pol] = 0.  After all of it evals += 1.  agree keeps the last evaluation's values.
 * A single exact match is not a detection: noise alone yields one now and then (of the order of 8 * 23 / 2^23 per code,
 * polarity and evaluation).  The library reports, the caller decides; run >= 3 is a sensible "open".
 *
 * ROWS.  wr_dcs_reset(bank, row) zeroes row `row`: its chips, the open chip, agree, run, hits and evals; the clock goes
 * on.  A negative row resets all rows and sets the clock to 0.  wr_dcs_seek(bank, frame) is the same with the clock at
 * `frame`: for a bank that joins a running stream.  A row that a push leaves out (nrows < max_rows) is reset: the
 * resampler's convention.
 * Limits, each WR_ERR_ARG: max_rows from 1 to 65535; ncodes from 1 to 128; words below 2^23; step in [2^19, 2^28];
 * max_errors from 0 to 3; a push of at most 2^28 frames.
 * Left out on purpose: muting audio by code (the detector reports, the caller decides); a host-side C++ class (the
 * reference has none to mirror); per-receiver code lists (one list per bank); clock recovery beyond the eight phases;
 * time sharding. */
int wr_dcs_word(unsigned int code, unsigned int *word);
int wr_dcs_step(unsigned int audio_rate, unsigned int *step);
/* words_host[ncodes]: 23-bit words (wr_dcs_word, or the caller's own); step: wr_dcs_step's. */
int wr_dcs_create(wr_dcs **bank, wr_dev *dev, unsigned int max_rows, const unsigned int *words_host, unsigned int ncodes,
                  unsigned int step, unsigned int max_errors);
int wr_dcs_destroy(wr_dcs *bank);
/* What a caller does for the row after wr_chan_reset_history or a retune of the receiver in that slot (and for all rows,
 * with wr_dcs_seek where the stream runs on, after wr_tuner_seek): the bank does not watch the tuner.  Asynchronous on the
 * device's stream. */
int wr_dcs_reset(wr_dcs *bank, int row);
int wr_dcs_seek(wr_dcs *bank, unsigned long long frame);
/* THE RULE on a plain block of rows in device memory: `nrows` rows of `nframes` floats, `row_stride` floats apart; row r of
 * the call is row r of the bank, and N advances by nframes.  Consecutive calls continue the streams whatever the lengths.
 * Asynchronous on the device's stream (as many launches as the rows' rings of chip sums ask for: one, unless the push
 * holds more than 255 chips); counted by wr_block_kernel_calls.  WR_ERR_ARG: NULL arguments, nrows > max_rows,
 * row_stride < nframes with several rows, more than 2^28 frames. */
int wr_dcs_push_rows(wr_dcs *bank, const float *audio_dev, size_t row_stride, size_t nrows, size_t nframes);
/* Pushes the last submit's audio rows of every channel slot, the rows wr_tuner_tones_push takes and counted as it counts
 * them (*slots: whole lane groups of 64); rows of slots that hold no channel carry no meaning.  The slicer's threshold
 * makes the result independent of af_gain, scale and the demodulator's DC.  Like every getter it sends held blocks out,
 * launches a pending post stage and closes an open streaming launch; it changes nothing the next block depends on.
 * WR_ERR_STATE: nothing submitted yet, several rate groups, the same submit pushed twice.  WR_ERR_ARG: max_rows below the
 * slot count, a bank of another device. */
int wr_tuner_dcs_push(wr_tuner *tuner, wr_dcs *bank, unsigned int *slots);
/* agree_host: uint8 [rows][ncodes][2]; run_host: uint32 [rows][ncodes][2]; hits_host: uint64 [rows][ncodes][2];
 * evals_host: uint64 [rows]; *rows = max_rows.  Any array may be NULL, all four NULL is WR_ERR_ARG.  Waits for the
 * device's stream. */
int wr_dcs_read(wr_dcs *bank, unsigned char *agree_host, unsigned int *run_host, unsigned long long *hits_host,
                unsigned long long *evals_host, unsigned int *rows);
/* What the bank was created with, and N.  Any pointer may be NULL.  Host only. */
int wr_dcs_info(wr_dcs *bank, unsigned int *ncodes, unsigned int *step, unsigned int *max_errors, unsigned long long *frames);

/* RESAMPLER: every receiver's audio at a sound-card rate.  A tuner's audio rate is what its decimations leave (50 kHz off
 * 100 Msps with 400 and 5; 32 kHz in BASELINE config 1); the reference avoids the question by choosing a tuner rate that
 * divides down to 48 000 (radio.cxx:79-81), which a 100 Msps front end does not have.  A bank is `max_rows` rows with ONE
 * rational ratio L / M and P taps per phase: a polyphase FIR run over plain rows of audio, or over the last submit's audio
 * rows of every channel slot of a tuner, in one launch sequence.
 *
 * THE RULE is this library's own definition, as the ones of af_gain, squelch, AGC and the tones are.
 * The bank has ONE clock: N, the input frames pushed since creation or since a reset of every row.  Every push advances
 * all rows together, so all rows of a push yield the same number of output frames and the receivers stay aligned.
 * A row holds the stream x[n]; x[n] = 0 for n < 0 and for frames before the row's last reset.  Each input is cleaned:
 *   x'   = 0.0f if (bits(x) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else min(max(x, -65536.0f), 65536.0f)
 * (-0.0f stays -0.0f).  Output frame m = 0, 1, ... has t = m * M, n0 = t / L (floor), ph = t mod L and
 *   acc  = +0.0f
 *   for k = 0 ... P-1 in this order:  acc = acc + c[ph][k] * x'[n0 - k]
 *   y[m] = acc
 * Every product and every sum is rounded to float32 once; nothing is fused, and there is one accumulator.  Taps are finite
 * and |c| <= 16 (wr_resamp_create refuses others), so |acc| <= 2^26: nothing overflows and no NaN arises.
 * Frame m comes out with the push that holds input frame n0(m): a push that takes the clock from N0 to N1 yields
 * ceil(N1 * L / M) - ceil(N0 * L / M) frames, which can be 0.  Only N mod M is needed and kept, so nothing ever wraps; two
 * 64-bit counts of frames in and out are kept beside it (wr_resamp_info).  A row's state is its last P - 1 cleaned inputs.
 * An output has ONE value whatever the grid and whatever the cut of the stream into pushes; a restatement in float32 numpy
 * is bit-identical.  The group delay is (L * P - 1) / 2 samples at L times the input rate: about P / 2 input frames.
 * Limits, each WR_ERR_ARG: 1 <= L <= 1024; 1 <= M <= 8 L and L <= 8 M (more decimation than that belongs to the tuner's
 * own filters); P a multiple of 4 from 4 to 64; L * P <= 16384; max_rows from 1 to 65535; a push of at most 2^28 frames;
 * input and output of a push may not overlap.
 * Left out on purpose: an int16 output; a host-side C++ class (the reference has none to mirror); per-row ratios; arbitrary
 * (non-rational) ratios and clock-drift tracking; resampling inside the streaming launch; time sharding.
 *
 * wr_resamp_ratio: *L = out_rate / g, *M = in_rate / g with g = gcd(in_rate, out_rate); needs no device.  WR_ERR_ARG: a
 * rate of 0, a NULL pointer (the limits above are wr_resamp_design's and wr_resamp_create's to enforce). */
int wr_resamp_ratio(unsigned int in_rate, unsigned int out_rate, unsigned int *L, unsigned int *M);
/* A Kaiser-windowed sinc for in_rate -> out_rate with P taps per phase, computed in double; needs no device.  beta = 8,
 * Nh = L * P taps at L * in_rate, transition width D = 5 * in_rate / P Hz centred at fc = min(in_rate, out_rate) / 2 - D / 2:
 *   h[i] = sinc(2 fc / (L in_rate) * (i - (Nh - 1) / 2)) * kaiser(i),   sinc(x) = sin(pi x) / (pi x),
 *   kaiser(i) = I0(beta * sqrt(1 - (2 i / (Nh - 1) - 1)^2)) / I0(beta)
 * scaled so that sum h = L, rounded to float32 once and stored as c[ph][k] = h[k * L + ph].  The stopband (from min / 2
 * up) lies below -65 dB, the passband (to min / 2 - D) within -60 dB of 1.  WR_ERR_ARG: a limit above, or unless
 * min(in_rate, out_rate) > 10 * in_rate / P (the passband edge would not lie above 0).  L and M may be NULL. */
int wr_resamp_design(unsigned int in_rate, unsigned int out_rate, unsigned int P, float *taps_host /* [L][P] */,
                     unsigned int *L, unsigned int *M);
/* taps_host[L][P] as wr_resamp_design stores them (or the caller's own).  WR_ERR_ARG: a limit above, a tap that is not
 * finite or whose magnitude exceeds 16. */
int wr_resamp_create(wr_resamp **rs, wr_dev *dev, unsigned int max_rows, unsigned int L, unsigned int M, unsigned int P,
                     const float *taps_host);
int wr_resamp_destroy(wr_resamp *rs);
/* Clears the row's history: it holds silence before its next frame; the clock runs on.  row < 0: every history, and the
 * clock returns to 0 (the frame counts too).  What a caller does after wr_tuner_seek, wr_chan_reset_history or a retune of
 * the receiver in that slot: the bank does not watch the tuner.  Asynchronous on the device's stream. */
int wr_resamp_reset(wr_resamp *rs, int row);
/* *n_out: the output frames a push of `nframes` frames would yield now.  Host only. */
int wr_resamp_out_frames(wr_resamp *rs, size_t nframes, size_t *n_out);
/* The rule on a plain block of rows in device memory: `nrows` rows of `nframes` floats, `row_stride` floats apart; row r of
 * the call is row r of the bank, and its *n_out output frames go to out_dev + r * out_stride.  Consecutive calls continue
 * the streams whatever the lengths.  A push of nrows < max_rows clears the histories of the rows it leaves out: those rows
 * saw nothing.  Asynchronous on the device's stream, *n_out is known without a wait; counted by wr_block_kernel_calls.
 * WR_ERR_ARG: NULL arguments, nrows > max_rows, row_stride < nframes or out_stride < *n_out with several rows, more than
 * 2^28 frames, input and output that overlap. */
int wr_resamp_push_rows(wr_resamp *rs, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                        size_t out_stride, size_t *n_out);
/* The ratio, the taps per phase and the frames pushed and yielded since creation or the last reset of every row.  Any
 * pointer may be NULL.  Host only. */
int wr_resamp_info(wr_resamp *rs, unsigned int *L, unsigned int *M, unsigned int *P, unsigned long long *frames_in,
                   unsigned long long *frames_out);
/* Pushes the last submit's audio rows of every channel slot: WR_STAGE_AUDIO as wr_tuner_audio_dev shows it -- after
 * squelch, AGC, af_gain and scale; row = wr_chan_slot, rows counted as wr_tuner_tones_push counts them (*slots: whole
 * lane groups of 64); rows of slots that hold no channel carry no meaning.  Row s yields *n_out frames at
 * out_dev + s * out_stride.  Like every getter it sends held blocks out, launches a pending post stage and closes an
 * open streaming launch; it writes nothing the next block reads.  Asynchronous behind that.
 * WR_ERR_STATE: nothing submitted yet, several rate groups, the same submit pushed twice (the bank remembers the tuner's
 * submit count).  WR_ERR_ARG: max_rows below the slot count, a bank of another device, out_stride < *n_out. */
int wr_tuner_resamp_push(wr_tuner *tuner, wr_resamp *rs, float *out_dev, size_t out_stride, size_t *n_out,
                         unsigned int *slots);

/* VOICE BANK: the stage between "decoded" and "listenable" -- per-receiver audio filters and a mute, in one launch.  NFM wants
 * de-emphasis (FM noise rises 6 dB per octave), the sub-audible tone or DCS word that the tone and DCS banks report is still
 * in the audio at 10-15 % of full deviation, AM audio carries its carrier as DC and SSB audio has no voice band-pass; the
 * banks' "it reports, the caller mutes" needs something on the device to mute with.  The reference has nothing of the kind.
 * A bank is `max_rows` rows, a table of F long FIR filters of ONE length T, and one control word per row that picks the
 * row's filter and mutes it.  De-emphasis, the tone high-pass and the voice low-pass fold into one linear-phase filter
 * (wr_voice_design); 512 to 2048 taps at 16 to 50 kHz do the job.  It is deliberately a bank of FIR filters and not of
 * recursive ones: an output is a fixed-order sum, independent of every other output.
 *
 * THE RULE is this library's own definition, as the ones of af_gain, squelch, AGC, the tones and the resampler are.
 * A bank has max_rows rows, from 1 to 65535; F filters, from 1 to 16; ONE length T for all filters, a multiple of 4 from 8
 * to 2048; taps c[f][k], finite and |c| <= 16 (wr_voice_create refuses others).  Every row has one 32-bit control word:
 * bits 0-7 hold the row's filter index, which must be below F; bit 8 is the mute flag; every other bit must be 0; the
 * default is 0.
 * A row holds the stream x[n]; x[n] = 0 for n < 0 and for frames before the row's last reset.  Each input is cleaned
 * exactly as the resampler cleans it:
 *   x'   = 0.0f if (bits(x) & 0x7fffffff) >= 0x7f800000 (inf, NaN), else min(max(x, -65536.0f), 65536.0f)
 * (-0.0f stays -0.0f; subnormals are not flushed).  One output frame comes out per input frame; with f the row's filter:
 *   acc  = +0.0f
 *   for k = 0 ... T-1 in this order:  acc = acc + c[f][k] * x'[n - k]
 *   y[n] = mute ? +0.0f : acc
 * Every product and every sum is rounded to float32 once; nothing is fused, and there is one accumulator.
 * |acc| <= 2048 * 16 * 65536 = 2^31, so nothing overflows and no NaN arises.  An output has ONE value whatever the grid and
 * whatever the cut of the stream into pushes; a restatement in float32 numpy is bit-identical.
 * A muted row's history runs on: un-muting gives the frames the row would have given.  A row's state is its last T - 1
 * cleaned inputs, so a change of the filter index applies the new taps to the old inputs from the next push on.  A push of
 * nrows < max_rows clears the histories of the rows it leaves out.  Input and output of a push may not overlap.  A push
 * takes at most 2^28 frames.  A 64-bit count of the frames pushed since creation or the last reset of every row is kept
 * (wr_voice_info).
 * Left out on purpose: recursive filters; per-row filter lengths; filtering inside the streaming launch; a host-side C++
 * class (the reference has none to mirror); an int16 output; time sharding.
 * The output is a plain block of rows: it goes straight into wr_resamp_push_rows.  The bank can just as well run BEHIND
 * the resampler, on its output rows at the lower rate, where a filter of the same sharpness is shorter (512 taps at 16 kHz
 * for 1024 at 32 kHz): both orders work, and the second is the cheap one.
 *
 * wr_voice_design: one filter of T taps for audio at `audio_rate`, computed in double; needs no device.  N = T - 1 taps, an
 * odd length, symmetric about d = T / 2 - 1, and tap T - 1 = +0: the group delay is exactly d frames, and a unit impulse at
 * k = d is the "no filter" entry of a table that stays aligned with the filtered rows.  On a grid of G = 32768 points
 * f_g = g * audio_rate / G:
 *   band(f) = (highpass_hz == 0 or f >= highpass_hz) and (lowpass_hz == 0 or f <= lowpass_hz)
 *   de(f)   = 1 if deemph_us == 0, else sqrt((1 + (2 pi 1000 tau)^2) / (1 + (2 pi f tau)^2)), tau = deemph_us * 1e-6
 *   D(g)    = band(f_g) * de(f_g)                               (de-emphasis has unity gain at 1 kHz)
 *   h[i]    = (1 / G) [D(0) + 2 sum_{g = 1}^{G / 2 - 1} D(g) cos(2 pi g (i - d) / G) + D(G / 2) cos(pi (i - d))] * kaiser(i)
 *   kaiser(i) = I0(beta * sqrt(1 - (2 i / (N - 1) - 1)^2)) / I0(beta),   beta = 6,   i = 0 ... N - 1
 * each tap rounded to float32 once, h[i] and h[N - 1 - i] with the same bits.  The edges are -6 dB points; the transition
 * half-width on each side is W = (beta / 0.1102 + 8.7 - 8) / (2.285 * 2 pi * (T - 1)) * audio_rate, about
 * 3.84 * audio_rate / (T - 1).  For 300 .. 3000 Hz (3400 at 8 kHz) with 750 us at 50 kHz / 1024 and 2048 taps and at
 * 32 kHz / 1024, without de-emphasis at 16 kHz / 512 and 8 kHz / 256, and for the high-pass alone at 50 kHz / 1024: |H| <= -55 dB
 * from highpass_hz - W down and from lowpass_hz + W up, and |H / D - 1| <= -45 dB between highpass_hz + W and lowpass_hz - W.
 * Shorter filters with de-emphasis at 50 kHz are not among these: at 512 taps they reach only -40 dB, because the 750 us
 * response is cut short.  WR_ERR_ARG, and nothing written: a rate of 0; T not a multiple of 4 from 8 to 2048; an edge at or
 * above audio_rate / 2; both edges given and highpass_hz + W >= lowpass_hz - W; deemph_us > 10000. */
int wr_voice_design(unsigned int audio_rate, unsigned int T, unsigned int highpass_hz, unsigned int lowpass_hz,
                    unsigned int deemph_us, float *taps_host /* [T] */);
/* taps_host[nfilt][T] as wr_voice_design stores them (or the caller's own).  WR_ERR_ARG: a limit above, a tap that is not
 * finite or whose magnitude exceeds 16. */
int wr_voice_create(wr_voice **bank, wr_dev *dev, unsigned int max_rows, unsigned int T, unsigned int nfilt,
                    const float *taps_host /* [nfilt][T] */);
int wr_voice_destroy(wr_voice *bank);
/* Clears the row's history: it holds silence before its next frame.  row < 0: every history, and the frame count returns to
 * 0.  The control words stay.  What a caller does after wr_tuner_seek, wr_chan_reset_history or a retune of the receiver in
 * that slot: the bank does not watch the tuner.  Asynchronous on the device's stream. */
int wr_voice_reset(wr_voice *bank, int row);
/* The control words of rows first ... first + n - 1.  Every word is validated before any changes: WR_ERR_ARG (and no row
 * changed) for a filter index that is not below F, a bit set beyond bits 0-8, rows that are not the bank's.  Synchronous;
 * ordered behind the pushes already on the device's stream, it takes effect with the next push. */
int wr_voice_set_rows(wr_voice *bank, unsigned int first, unsigned int n, const unsigned int *ctl_host);
/* ... as they were set last.  Host only. */
int wr_voice_get_rows(wr_voice *bank, unsigned int first, unsigned int n, unsigned int *ctl_host);
/* The rule on a plain block of rows in device memory: `nrows` rows of `nframes` floats, `row_stride` floats apart; row r of
 * the call is row r of the bank, and its nframes output frames go to out_dev + r * out_stride.  Consecutive calls continue
 * the streams whatever the lengths.  Asynchronous on the device's stream; counted by wr_block_kernel_calls.
 * WR_ERR_ARG: NULL arguments, nrows > max_rows, row_stride < nframes or out_stride < nframes with several rows, more than
 * 2^28 frames, input and output that overlap. */
int wr_voice_push_rows(wr_voice *bank, const float *in_dev, size_t row_stride, size_t nrows, size_t nframes, float *out_dev,
                       size_t out_stride);
/* Pushes the last submit's audio rows of every channel slot, the rows wr_tuner_resamp_push takes and counted as it counts
 * them (*slots: whole lane groups of 64); row s yields the submit's audio frames at out_dev + s * out_stride.  Like every
 * getter it sends held blocks out, launches a pending post stage and closes an open streaming launch; it writes nothing
 * the tuner reads.  Asynchronous behind that.
 * WR_ERR_STATE: nothing submitted yet, several rate groups, the same submit pushed twice.  WR_ERR_ARG: max_rows below the
 * slot count, a bank of another device, a NULL out_dev, out_stride below the frames, an output that overlaps the audio. */
int wr_tuner_voice_push(wr_tuner *tuner, wr_voice *bank, float *out_dev, size_t out_stride, unsigned int *slots);
/* The filter length, the filters and the frames pushed since creation or the last reset of every row.  Any pointer may be
 * NULL.  Host only. */
int wr_voice_info(wr_voice *bank, unsigned int *T, unsigned int *nfilt, unsigned long long *frames);
#ifdef __cplusplus
}
#endif
#endif /* WEBRADIO_AMD_H_ */
