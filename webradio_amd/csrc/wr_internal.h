/*
 * wr_internal.h -- internal C++ interface between the C ABI (wr_dev.hip, wr_tuner*.hip, wr_spectrum.hip, wr_banks.hip), the host
 * design math (wr_design.cpp) and the kernels (wr_kernels.hip, wr_fft.hip, wr_levels.hip, wr_agc.hip, wr_tones.hip,
 * wr_dcs.hip, wr_resamp.hip, wr_voice.hip).
 * Not installed; the public boundary is include/webradio_amd.h.
 */
#ifndef WR_INTERNAL_H_
#define WR_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "webradio_amd.h"
#include "wr_plan.h"                       /* launch geometry and the constants it depends on (WR_HIST, WR_SPLIT_N, WR_TAPSETS, ...) */

#define WR_MAX_DEVICES 64                  /* device indices the per-device tables of this library hold */

/* ---- what other translation units need of a wr_dev (wr_dev.hip, wr_tuner_submit.hip) ---- */
int         wrc_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   /* sets wr_last_error() */
int         wrc_dev_index(const wr_dev *dev);
hipStream_t wrc_dev_stream(const wr_dev *dev);
hipError_t  wrc_dev_stream_sync(wr_dev *d);               /* closes the streaming launch that is open on the device's stream, if any, and waits for the stream */
/* the event the tuner's last launch stamped on completion (wr_tuner_mark_launches), or NULL (wr_ring.hip) */
int         wrc_tuner_launch_mark(wr_tuner *t, hipEvent_t *ev);

/* ---- host design math (wr_design.cpp) ---- */
void     wrd_sin_table(float *table);
void     wrd_sin_table_rounded(float *table);
int      wrd_phase_step(int if_hz, unsigned int input_rate);
unsigned wrd_lowpass_maxbin(unsigned int fir_length, unsigned int passband, unsigned int input_rate);
void     wrd_lowpass_design(unsigned int fir_length, unsigned int passband, unsigned int input_rate, float *coeff);
void     wrd_spectrum_window(unsigned int n, float *window);
void     wrd_split_tables(float *hi_cs /* [256][2] cos,sin */, float *lo_cs /* [256][2] */);
void     wrd_twiddles(unsigned int n, float *tw /* [n/2][2] cos,-sin of 2*pi*k/n */);
/* wr_agc_design's arithmetic (in double); non-zero: an argument is a NaN or out of range, or the floor would be subnormal */
int      wrd_agc_design(float target_dbfs, float decay_db_per_s, float max_gain_db, unsigned int audio_rate, float *target,
                        unsigned int *floor_bits, unsigned int *step);
/* wr_tone_step's arithmetic (in double); non-zero unless 0 < hz < audio_rate / 2 */
int      wrd_tone_step(double hz, unsigned int audio_rate, unsigned int *step);
/* wr_resamp_ratio's and wr_resamp_design's arithmetic, and the header's limits on (L, M, P); non-zero: refused */
int      wrd_resamp_ratio(unsigned int in_rate, unsigned int out_rate, unsigned int *L, unsigned int *M);
int      wrd_resamp_limits(unsigned int L, unsigned int M, unsigned int P);
int      wrd_resamp_design(unsigned int in_rate, unsigned int out_rate, unsigned int P, float *taps /* [L][P] */, unsigned int *L,
                           unsigned int *M);
/* wr_voice_design's arithmetic (in double); non-zero: refused, and nothing written */
int      wrd_voice_design(unsigned int audio_rate, unsigned int T, unsigned int highpass_hz, unsigned int lowpass_hz,
                          unsigned int deemph_us, float *taps /* [T] */);

/* ---- per-slot parameter block of one rate group of a tuner, device SoA ---- */
struct WrGroupDev {
	/* all arrays have `slots` entries (slots is a multiple of 64) unless noted */
	/* the arrays a block CHANGES come as two sets: a launch reads set `sp` and writes set
	 * `sp ^ 1`, so consecutive blocks' DDC launches depend only on each other */
	unsigned int *phase[2];     /* left-aligned phase at block start: DownConverter::phase << 1 */
	unsigned int *step;         /* phaseStep << 1 (two's complement) for this block */
	float        *hist_cs[2];   /* [63][slots][2] LO (cos, sin) each of the last 63 input frames was mixed with;
	                               WR_NCO_ROTATE: the TURN (cos, sin) into frame r - 62 of the next block */
	float        *hist_lo[2];   /* WR_NCO_ROTATE only: [63][slots][2] the LO values (segment anchors) */
	int          *flags;        /* bit0: slot active (host-written only) */
	int          *mode;         /* wr_mode, or -1 for an idle slot (what the post-DDC kernels test) */
	float        *taps1;        /* [64][slots] channel-filter taps, taps1[j*slots+s] = coeff[j] */
	float        *taps2;        /* [l2][slots] audio-filter taps (l2 = 64, or 128 / 256: below) */
	float        *taps2u;       /* [lane groups][l2] the group's one audio filter, where its channels share one
	                               (WrTunerLaunch::uniform2_mask) */
	/* what a DDC wave needs before its first tap, laid out so that it is ONE coalesced load each (a
	 * wave that gathers them -- 64 tap rows, four table entries per lane -- queues 320 cache-line
	 * requests behind the other 31 waves of its CU, and every wave of the launch does so at once) */
	float        *rot;          /* WR_NCO_ROTATE: [slots][4] the two turns of the slot's step:
	                               cis(2 pi S / 65536), cis(2 pi (S+1) / 65536), S = step >> 16 */
	float        *taps1u;       /* [groups][WR_TAPSETS][64] the distinct channel filters of lane group g (when
	                               there are at most WR_TAPSETS): taps1u[(g*WR_TAPSETS + q)*64 + j] =
	                               coeff_q[63 - j], the tap of window sample j */
	int          *tapsel;       /* [slots] which of its group's filters the slot's channel uses */
	/* optional SECOND channel-filter stage between the DDC and the demodulator (one
	 * 64-tap stage cannot cut a 12.5 kHz channel out of a 100 Msps stream, lowpass.cxx:167 gives bin 0) */
	float        *taps1b;       /* [64][slots] its taps */
	float        *iq2_hist[2];  /* [63][slots][2] its history: the last 63 first-stage frames; ping-pong */
	float        *chan_iq2[2];  /* [k1max / d1b][slots][2] its output = the demodulator's input */
	/* receiver controls the reference only stubs (receiverhandler.cxx:112,118-119,127) */
	/* a channel filter of MORE than 64 taps (128 or 256; the rate group is keyed by the length too): its taps
	 * and, as LowPass::block does (lowpass.cxx:138-142), the last L - 1 MIXED frames of every channel */
	float        *taps1L;       /* [L][slots] */
	float        *mixhist[2];   /* [L - 1][slots][2], ping-pong with the state set */
	float        *gain;         /* [slots] af_gain as a factor (1 = 0 dB) */
	float        *squelch;      /* [slots] squelch threshold as a power (0 = open) */
	float        *prev_iq[2];   /* [slots][2] Demodulator::prev_i/prev_q, ping-pong by block parity */
	float        *chan_iq[2];   /* [k1max][slots][2] channel-filter output, time major; double buffered so
	                               that block b+1's DDC can run while block b is being demodulated */
	float        *dem[2];       /* [63 + k1max][slots] demod output, 63 history rows in front; ping-pong */
	float        *audio;        /* [slots][k2max] audio, channel major */
	float        *audio_set[4]; /* four arrays of that shape, `audio` one of them: inside a streaming launch the blocks' post stages store
	                               by turns (block j into set member (first + j) mod 4), so that blocks whose post-stage tasks run side by
	                               side never store into the same array; the stream's close makes the array its last block wrote
	                               `audio` (wr_tuner_stream.hip: wrc_stream_close) */
	/* taps of the group's audio filter and of its second channel stage: 64, or 128 / 256 (the rate group is keyed by
	 * them; dem then carries l2 - 1 history rows, iq2_hist l1b - 1, taps2 / taps1b l2 / l1b rows) */
	unsigned int  l2 = 64, l1b = 64;
};

struct WrTunerLaunch {
	const float *cur;           /* this block's IQ, nframes frames (device), or NULL when ... */
	const uint8_t *cur_u8;      /* ... the block is in the RTL-SDR byte format (2 bytes per frame) */
	const float *hist;          /* last 63 IQ frames of the previous block (device) */
	float       *hist_next;     /* receives the history for the next block */
	int          parity;        /* which of the group's prev_iq / dem ping-pong buffers is current */
	int          sp;            /* which state set (phase, LO history) this block reads */
	int          cb;            /* which chan_iq buffer this block writes */
	size_t       nframes;
	unsigned int d1, d2;
	unsigned int slots;         /* row stride of every per-slot array */
	unsigned int slots_used;    /* slots [0, slots_used) hold channels (multiple of 64) */
	size_t       k1, k2;        /* frames per channel at channel / audio rate for this block */
	size_t       k2max;         /* channel stride of audio */
	int          nco_mode;
	float        audio_scale;   /* multiplies the audio on store (1 = as the reference) */
	int          use_gain, use_squelch;   /* some channel has an af_gain / a squelch threshold set */
	unsigned long long uniform_mask;   /* bit g: all channels of lane group g share ONE channel filter */
	unsigned long long uniform2_mask;  /* bit g: ... and ONE audio filter (WrGroupDev::taps2u) */
	unsigned long long fewsets_mask;   /* bit g: lane group g has at most WR_TAPSETS distinct channel filters */
	unsigned char nsets[64];           /* distinct channel filters of lane group g (valid where fewsets_mask says) */
	int          one_filter;           /* every channel of the rate group uses ONE and the same channel filter */
	void        *ev_start, *ev_stop;   /* hipEvent_t pair the DDC launch itself stamps (profiling), or NULL */
	bool         seeking = false;      /* the first block after wr_tuner_seek: phase = frame * step in closed form, the state sets
	                                      handed to the launch are all-zero ones (wr_tuner_submit.hip: submit_group) */
	unsigned int seek_lo = 0;          /* the frame's low 32 bits */
};

/* ---- kernel launchers (wr_kernels.hip); all return hipError_t ---- */
/* hipFuncAttributeMaxDynamicSharedMemorySize is a per-device setting of the loaded code object: a process that drives several
 * GPUs (the host runtime gives every tuner its own) has to set it once on each.  `done` is the flag array of ONE kernel
 * instance, `bytes` the MOST that instance ever asks for.  Plain flags: two threads racing on a first call both set the
 * attribute, to the same value -- what every call did before there were flags. */
hipError_t allow_lds(const void *fn, size_t bytes, bool (&done)[WR_MAX_DEVICES]);
hipError_t wrk_mix(hipStream_t st, const float *in, float *out, size_t nframes,
                   unsigned int phase, int step, const float *table_dev);
hipError_t wrk_fir(hipStream_t st, const float *in, size_t nframes, unsigned int channels,
                   unsigned int decim, unsigned int fir_length, const float *coeff_dev, const float *hist_dev,
                   float *out);
hipError_t wrk_hist_update(hipStream_t st, const float *in, size_t nframes, unsigned int channels,
                           unsigned int fir_length, float *hist_dev, float *scratch_dev);
hipError_t wrk_demod(hipStream_t st, int mode, const float *in, size_t nframes, float prev_i,
                     float prev_q, float *out);
hipError_t wrk_u8_to_f32(hipStream_t st, const uint8_t *in, float *out, size_t count);
hipError_t wrk_stage_windows(hipStream_t st, const void *src_mapped, bool u8, float *dst, size_t nframes, unsigned int period,
                             unsigned int len, size_t tail_frames);

/* what one launch of the post stage (demodulator + audio filter of ONE block) works on */
struct WrPostArgs {
	const float *chan_iq;        /* [k1][slots][2] the block's channel IQ */
	unsigned int k1, slots;
	const int   *mode;
	const float *prev_iq;        /* [slots][2] frame before the block's first */
	float       *prev_next;
	const float *dem_hist;       /* [63][slots] audio filter history ([64 nseg - 1] rows) */
	float       *dem_hist_next;
	size_t       k2;
	unsigned int tiles;          /* tiles of POST_TK audio frames per lane group */
	unsigned int run;            /* consecutive tiles one workgroup takes */
	unsigned int ntiles;         /* workgroups per lane group = ceil(tiles / run), plus the one that writes the state */
	const float *taps2;
	const float *taps2u;         /* [groups][64 nseg], read through the scalar cache */
	unsigned long long uni2;     /* bit g: lane group g's channels share one audio filter (taps2u) */
	float       *audio;
	size_t       k2max;
	float        scale;
	unsigned int d2;
	unsigned int groups;         /* lane groups in use */
	const float *gain;           /* [slots] af_gain factors, or NULL: all 1 */
	const float *squelch;        /* [slots] squelch thresholds (power of the demodulator's input, mean over the
	                                d2 frames behind an audio frame), or NULL: all open */
	float       *audio_host;     /* r04: page-locked HOST memory (a slot of the tuner's audio ring, mapped) that gets every
	                                audio sample too, rows `host_stride` floats apart -- the block's audio is in the ring when
	                                the launch has run, no device-to-host copy behind it; NULL: device memory only */
	size_t       host_stride;
	unsigned int nseg = 1;       /* the audio filter's taps / 64: 1, or 2 / 4 (dem_hist then has 127 / 255 rows, taps2 128 / 256,
	                                taps2u [groups][taps]) */
	const float *chan_prev = nullptr;   /* r05 (the streaming launch): the channel IQ of the block BEFORE this one, [k1][slots][2], k1 >= 64 nseg --
	                                the 64 nseg - 1 rows of audio-filter history and the demodulator's previous frame are then made from
	                                ITS last 64 nseg rows (the same operations on the same frames: the same bits) instead of read
	                                from dem_hist / prev_iq, so that a block's post stage does not wait for the one before */
};
/* `post` (optional): the post stage of the PREVIOUS block, run by extra workgroups of the same
 * launch beside this block's DDC (only taken up by the ROTATE / uniform-taps kernel; *post_taken
 * says whether it was) */
/* WR_TUNE_DDC_NG2_MIN_PASSES: set (value < 0: default again) and/or read; returns the value in force before */
long wrk_tune_ng2_min_passes(long value, bool set);
hipError_t wrk_tuner_ddc(hipStream_t st, const WrTunerLaunch &L, const WrGroupDev &G,
                         const float *table_dev, const float *hi_dev, const float *lo_dev,
                         int num_cus, const WrPostArgs *post = nullptr, bool *post_taken = nullptr);
/* the same for a channel filter of `len` = 128 or 256 taps (k_tuner_ddc_long: the reference's arithmetic in every
 * nco mode); also rolls the group's state (phase, mixed history) into the other set */
hipError_t wrk_tuner_ddc_long(hipStream_t st, const WrTunerLaunch &L, const WrGroupDev &G, unsigned int len,
                              const float *table_dev, int num_cus, bool rotate, bool rotate_one_filter, const float *hi_dev,
                              const float *lo_dev, const WrPostArgs *post = nullptr, bool *post_taken = nullptr);
hipError_t wrk_tuner_demod(hipStream_t st, const WrTunerLaunch &L, const WrGroupDev &G);
/* second channel-filter stage: k1a first-stage frames of chan_iq[cb] -> k1a / d1b frames of chan_iq2[cb];
 * history from iq2_hist[p2], next history into iq2_hist[p2 ^ 1] */
hipError_t wrk_tuner_iq2(hipStream_t st, const WrGroupDev &G, unsigned int slots, unsigned int slots_used,
                         size_t k1a, unsigned int d1b, int cb, int p2);
hipError_t wrk_tuner_audio(hipStream_t st, const WrTunerLaunch &L, const WrGroupDev &G);
WrPostArgs wrk_post_args(const WrTunerLaunch &L, const WrGroupDev &G);
hipError_t wrk_tuner_post(hipStream_t st, const WrTunerLaunch &L, const WrGroupDev &G);
hipError_t wrk_tuner_post_args(hipStream_t st, const WrPostArgs &A);
bool wrk_tuner_post_supported(unsigned int d2);
hipError_t wrk_input_hist(hipStream_t st, const float *cur, const uint8_t *cur_u8, size_t nframes,
                          const float *hist, float *hist_next);
hipError_t wrk_seek(hipStream_t st, const WrGroupDev &G, unsigned int slots, int sp, int parity, int p2,
                    unsigned long long frame);
hipError_t wrk_gather_rows(hipStream_t st, const float *src, size_t rows, size_t row_stride_floats,
                           size_t col_offset_floats, unsigned int width_floats, float *dst);

/* ---- the streaming launch (r05; wr_tuner_set_streaming): ONE persistent launch of the fused path that takes the
 * tuner's blocks as they are submitted -- the host rings a doorbell in page-locked memory instead of launching a
 * kernel per block, so a launch's ramp and tail (about 4.6 us at C2: every wave's state, the LDS tables, the first
 * windows; the ragged end) are paid once per STREAM, not once per block, and a block's post stage starts the moment
 * its last channel-IQ row is out, whether or not another block follows (dsp/dspblock.cxx:169-212: a block's output
 * leaves within its own run()).  See k_tuner_stream in wr_kernels.hip. ---- */
#define WR_STREAM_MAXJ   WR_STREAM_MAX_BLOCKS             /* blocks one streaming launch takes at most (the host then opens the next) */
#define WR_STREAM_RING   6u                /* blocks of channel IQ the ring between the DDC waves and the post stage holds.  r06: 6,
                                              not 8 -- the launch runs at the package's power limit (profiles/r06_power.txt) and the
                                              channel IQ's way to memory and back is a seventh of what it spends; 123 MB of ring
                                              (C2) beside the input windows stay in the 256 MB Infinity Cache where 164 MB did not
                                              quite: 29.8-30.0 against 30.5-30.7 us per block, 33.0-33.9 against 34.2-34.4 at the
                                              driver's 20 steps, two boxes; 5 and 4 leave the DDC too little room to run ahead */
struct WrStreamDesc {                      /* one submitted block */
	unsigned long long cur;                /* device address of its frames (float pairs, or byte pairs) */
	unsigned long long audio_host;         /* mapped page-locked ring slot that takes its audio too, or 0 */
	unsigned int count;                    /* r06: blocks rung with this one = its index + 1: the 4 bytes a device-side doorbell copies
	                                          into WrStreamDev::ready_up (they must lie in page-locked memory until the copy has run) */
	unsigned int pad;
};
struct WrStreamCtl {                       /* page-locked host memory, mapped: the doorbell and the way back */
	volatile unsigned int ready;           /* host -> device: blocks submitted so far (monotonic) */
	volatile unsigned int stop;            /* host -> device: 1 = `ready` is final */
	volatile unsigned int pad0[14];
	volatile unsigned int done;            /* device -> host: blocks whose audio is complete */
	volatile unsigned int final_blocks;    /* device -> host, at exit: blocks the launch processed */
	volatile unsigned int err;             /* device -> host: non-zero = a wait ran into its deadline (WR_STREAM_ERR_*) */
	volatile unsigned int self_closed;     /* device -> host: the doorbell was silent for `idle_ticks`: closed on its own */
	volatile unsigned int long_blocks;     /* device -> host (r06): blocks whose post stage went in the LONG runs of tiles (the host was ahead) */
	volatile unsigned int pad1[11];
};
#define WR_STREAM_SHARDS 16u               /* counters a block's DDC completions are spread over, a cache line each */
struct WrStreamDev {                       /* device memory: what the bell wave republishes, and the hand-over counters */
	unsigned int ready, stop;
	unsigned long long beat;                   /* the bell's heartbeat: the 100 MHz clock, every time round its loop */
	unsigned int ready_up;                     /* r06: the doorbell's device-side twin, written by a copy on the upload stream behind a
	                                              block's own copy (blocks out of page-locked host memory); the bell takes the larger */
	unsigned int pad0[27];
	/* what the waiting waves poll: one word each, written once per block (never the counters the arrivals land on:
	 * 4 000 waves arriving on ONE word queue up at 11-13 ns each -- MI355X_MICROARCH.md "fanin" -- and every wave
	 * that has an arrival in flight waits for it the next time it waits for vector memory) */
	unsigned long long progress;               /* low word: blocks whose channel IQ is complete; high word: blocks whose post
	                                              stage is complete, in order.  ONE writer (the watcher wave), one 8-byte store:
	                                              a DDC wave entering a block learns both with one load */
	unsigned int drain_from;                   /* 0, or 1 + the first block whose post-stage tasks are handed out by TICKET (post_ticket)
	                                              instead of by workgroup index: the watcher sets it when it learns that the stream is
	                                              closed, to a block nobody can have begun (its channel IQ is not complete yet) -- from
	                                              there on the DDC workgroups, which have nothing left to do, take post tasks too */
	unsigned int pad1[29];
	unsigned int post_done[WR_STREAM_MAXJ];    /* post-stage TASKS of block j that are finished (their stores released) */
	unsigned int post_fine[WR_STREAM_MAXJ];    /* r06: 1 = block j's post stage goes in the SHORT runs of tiles (WrStreamArgs::drain_run): the watcher
	                                              decides when the block's channel IQ is complete -- short unless two further blocks are rung
	                                              already (the host is ahead: what counts is what a block costs, not how soon its audio is out) */
	unsigned int post_ticket[WR_STREAM_MAXJ];  /* the next task of block j to hand out (blocks from drain_from on) */
	unsigned int ddc_done[WR_STREAM_MAXJ][WR_STREAM_SHARDS][32];   /* lane-group units of block j whose channel IQ is in memory:
	                                              the sum over the shards' first words (wave w arrives on shard w mod SHARDS) */
	WrStreamDesc desc[WR_STREAM_MAXJ];
	unsigned long long cur[WR_STREAM_MAXJ + 1u];   /* cur[j + 1] = where block j lies, cur[0] = 0: a block's address and its
	                                              predecessor's side by side */
};
struct WrStreamArgs {
	/* control */
	WrStreamCtl        *ctl;               /* mapped host memory */
	const WrStreamDesc *desc_host;         /* mapped host memory, [WR_STREAM_MAXJ] */
	WrStreamDev        *sdev;
	unsigned long long  idle_ticks;        /* 100 MHz ticks without a bell after which the launch closes itself */
	unsigned long long  wait_ticks;        /* ... any other wait may take before it gives up (an error) */
	unsigned int        n_ddc, n_post;     /* workgroups per role; one more rings the bell */
	unsigned long long *tl;                /* -DSTREAM_TL builds with WR_STREAM_TL=1: [wave][8] cycle counts of the DDC waves
	                                          (development aid; wr_debug_stream_tl) */
	unsigned long long  cur0, audio0;      /* block 0's descriptor (the launch exists because of it): here, not copied to
	                                          device memory ahead of the launch -- two small copies on the stream cost the
	                                          open 25 us; the bell wave puts it into WrStreamDev for whoever needs it later */
	/* the block shape (every block of a stream has it) */
	unsigned long long  nframes;           /* input frames per block, = k1 * d1 */
	unsigned int        k1, d1, is_u8;
	unsigned int        ext;               /* r06: blocks may be written by the DMA engine while the launch runs: window loads at agent scope */
	unsigned int        slots, groups;     /* row stride of the per-slot arrays; lane groups in use */
	unsigned long long  gmap0, gmap1;      /* which lane groups (as k_tuner_ddc) */
	unsigned int        kslow;             /* output frames of a block whose window reaches into the block before */
	unsigned int        kmax;              /* the most distinct channel filters a lane group of the launch mixes, 1..WR_TAPSETS
	                                          (it and one_filter fill alignment holes: no other field moves, nor does the
	                                          kernel's argument block grow) */
	/* the DDC's state (WrGroupDev), set `sp` read, set `sp ^ 1` written at exit */
	const float        *hist;              /* tuner input history [63][2] before block 0 */
	float              *hist_next;
	const unsigned int *phase, *step;
	unsigned int       *phase_next;
	const float        *hist_cs, *hist_lo;
	float              *hist_cs_next, *hist_lo_next;
	const int          *flags;
	const float        *taps1, *rot, *taps1u;
	const int          *tapsel;
	const float        *table, *hi_cs, *lo_cs;
	float              *ring;              /* [WR_STREAM_RING * k1][slots][2] channel IQ */
	float              *audio_bufs[4];     /* WrGroupDev::audio_set, from the current one on: block j's device audio goes to audio_bufs[j & 3] */
	/* the post stage: what wrk_post_args gives for ONE block, and the two ping-pong state sets */
	WrPostArgs          post;
	unsigned int        drain_run, drain_ntiles;   /* r06: `post.run` / `post.ntiles` for the blocks that go in short runs (WrStreamDev::post_fine:
	                                          a host-paced stream, and a closed stream's last blocks) -- there a block's end is latency, not energy */
	const float        *prev_iq[2];
	float              *dem[2];
	int                 parity0;           /* set block 0 reads */
	unsigned int        one_filter;        /* ONE channel filter for every channel (WrTunerLaunch::one_filter) */
};
#define WR_STREAM_ERR_WAIT   1u            /* a wait inside the launch ran into `wait_ticks` */
/* workgroups the launch needs co-resident (it sizes its roles to them); 0 = this launch shape cannot stream */
/* (`nseg`: the audio filter's taps / 64 -- 1, 2, or 4 up to an audio decimation of 3) */
hipError_t wrk_stream_geometry(unsigned int d2, unsigned int groups, unsigned int kmax, bool one_filter, unsigned int nseg,
                               int num_cus, unsigned int *n_ddc, unsigned int *n_post);
hipError_t wrk_tuner_stream(hipStream_t st, const WrStreamArgs &A, void *ev_start, void *ev_stop);

/* ---- FFT (wr_fft.hip) ---- */
struct WrFftPlan {
	unsigned int n;             /* frame size */
	unsigned int channels;      /* 2: IQ frames; 1: real samples, transformed as n/2 packed points and untangled */
	WrFftShape shape;           /* wrp_fft_shape(n, channels): the points that are transformed, n1 * n2 of them, and the path */
	float *tw_n;                /* [n/2][2] twiddles of the frame size (device) */
	float *tw_sub;              /* [shape.sub/2][2] twiddles of the LDS sub-transforms (device); single-pass: unused */
	float *window;              /* [n] (device) */
	float *window_p1;           /* WR_FFT_REG64K: the window in the order k_fft64k_pass1's threads take it, else NULL */
	float *work;                /* [work_frames][n][2] (device): the intermediate between the passes of the frames in flight; real:
	                               half of it is that, half the packed transform in front of the untangle step
	                               (wrp_fft_untangle_offset).  Single-pass: NULL */
	size_t work_frames;         /* one from create on, more after wrk_fft_plan_reserve; single-pass: 0 */
};
/* the tables and a work area of one frame; on failure the plan is freed again.  Synchronous copies: the caller has settled
 * the device's stream */
hipError_t wrk_fft_plan_create(WrFftPlan *P, unsigned int n, unsigned int channels);
void       wrk_fft_plan_free(WrFftPlan *P);
/* room in the work area for a call of `frames` frames, as far as wrp_fft_work_frames gives it; growing waits for `dev`'s stream */
hipError_t wrk_fft_plan_reserve(WrFftPlan *P, size_t frames, wr_dev *dev);
/* frame f starts `f * hop` frames (of P.channels floats) into `iq` */
hipError_t wrk_fft_frames(hipStream_t st, const WrFftPlan &P, const float *iq, size_t hop,
                          size_t nframes_fft, float *bins_out /* or NULL */, float *db_out /* or NULL */);
/* `ngroups` groups of `nframes_fft` frames: frame f of group g starts `g * gstride + f * hop` frames into `iq`, its row is
 * row g * nframes_fft + f.  Single-workgroup sizes: one launch for all groups; two-pass sizes: a loop over the groups */
hipError_t wrk_fft_groups(hipStream_t st, const WrFftPlan &P, const float *iq, size_t hop, size_t nframes_fft, size_t ngroups,
                          size_t gstride, float *bins_out /* or NULL */, float *db_out /* or NULL */);
/* wr_spectrum_batch_avg's reduction (k_spec_reduce) of a chunk's bins[groups][frames][n][2]; `carry`: [groups][n][2], read
 * unless `first`, written unless `last`; `nframes_fft`: the frames of a whole group, the mean's divisor */
hipError_t wrk_spec_reduce(hipStream_t st, const float *bins, unsigned int n, size_t groups, size_t frames, bool first, bool last,
                           float *carry, size_t nframes_fft, int linear, float *mean /* or NULL */, float *peak /* or NULL */);
/* k_waterfall_row's reduction and palette on `nrows` shifted dB rows of n floats in device memory */
hipError_t wrk_rows_waterfall(hipStream_t st, const float *db, unsigned int n, size_t nrows, unsigned int width, int hold,
                              float *db_rows /* or NULL */, uint8_t *palette /* or NULL */);
/* wr_detect.hip: one chunk of wr_spectrum_rows_detect -- `nrows` (plan.chunk_rows at most) rows of n floats: k_detect_floor into
 * floors[nrows][plan.nspans], k_detect_segments into det[nrows][max_det] and count[nrows]; `rule` has passed wrp_detect_rule_bad */
hipError_t wrk_detect_rows(hipStream_t st, const float *rows, unsigned int n, size_t nrows, const wr_detect_rule *rule,
                           const WrDetectPlan &plan, unsigned int max_det, wr_detection *det /* or NULL: max_det = 0 */,
                           unsigned int *count, float *floors);

/* the dB row (shifted) of rows [first, first + P.n) of the first `cols` columns of iq[rows][S][2], row of column s at
 * db + s * P.n: IQ plans of at most 8192 points, cols <= S a multiple of 64 */
hipError_t wrk_fft_cols(hipStream_t st, const WrFftPlan &P, const float *iq, unsigned int S, unsigned int cols, size_t first,
                        float *db, int num_cus /* of the device: columns share a workgroup only beyond that many */);

/* ---- signal levels (wr_levels.hip) ---- */
/* of the first `cols` columns of iq[k1][S][2]: *out = [3][cols] in `work` (room for wrk_chan_levels_work floats): the mean
 * of e = i*i + q*q (summed in runs of 16, groups of 16 runs, in order: a function of k1 alone), its peak, and -- with
 * `squelch` ([cols] thresholds as powers, 0 = open; else NULL) -- as unsigned the audio frames k < k2 that audio_out mutes
 * (the mean of e over rows k*d2 .. k*d2 + d2 - 1 below the threshold), 0 without.  cols <= S, any cols */
size_t     wrk_chan_levels_work(unsigned int cols, size_t k1);
hipError_t wrk_chan_levels(hipStream_t st, const float *iq, size_t S, unsigned int cols, size_t k1, unsigned int d2, size_t k2,
                           const float *squelch, float *work, const float **out);

/* ---- audio AGC (wr_agc.hip) ---- */
struct WrAgcPar {                          /* one row's parameters */
	float        target;               /* the level the peak is brought to, linear */
	unsigned int floor_bits;           /* the envelope's lower bound, as a float's bits: target / the largest gain */
	unsigned int step;                 /* what the envelope falls per frame, in units of a float's bit pattern; or one of: */
	float        af_gain;              /* the row's af_gain factor (applied behind the AGC) */
};
#define WR_AGC_OFF  0xffffffffu            /* step: a row without AGC -- it gets the call's scale and nothing else */
#define WR_AGC_IDLE 0xfffffffeu            /* step: a row that is nobody's (a tuner slot without a channel) -- left alone */
/* in place on `nrows` rows of `nframes` floats, `row_stride` floats apart: include/webradio_amd.h's rule (wr_agc_rows) with
 * par[row] and state[row] (read, and left as the row's last E), then `scale`; a workgroup per row */
hipError_t wrk_agc_rows(hipStream_t st, float *audio, size_t row_stride, size_t nrows, size_t nframes, const WrAgcPar *par,
                        unsigned int *state, float scale);

/* ---- tone bank (wr_tones.hip) ---- */
struct WrTonesRow {                        /* everything a bank holds of one row; all zero: a row that begins its stream */
	long long acc[WR_LANES][2];        /* I, Q of the open window, per tone */
	long long lat[WR_LANES][2];        /* I, Q of the last complete window */
	long long part[2][WR_LANES][2];    /* what a push's workgroups add up: [the last window that ends in it, the open one behind
	                                      it][tone][I, Q]; zero between pushes */
	long long acc_e, lat_e, part_e[2]; /* the same three for E */
	unsigned long long windows;        /* complete windows so far */
	unsigned int fill, pad;            /* frames in the open window, < window */
};
/* include/webradio_amd.h's rule (wr_tones_push_rows) on `nrows` rows of `nframes` floats, `row_stride` floats apart: row r
 * goes into rows[r]; t12[4096] is every 16th entry of the sine table, steps[64] the tones' phase steps (0 beyond ntones) */
hipError_t wrk_tones_push(hipStream_t st, const float *audio, size_t row_stride, size_t nrows, size_t nframes, WrTonesRow *rows,
                          const float *t12, const unsigned int *steps, unsigned int ntones, unsigned int window);

/* ---- DCS bank (wr_dcs.hip) ---- */
struct WrDcsRow {                          /* everything a bank holds of one row; all zero: a row that begins its stream */
	long long ring[WR_DCS_RING];       /* chip sums; the open chip among them */
	unsigned long long hits[WR_DCS_CODES][2];
	unsigned long long evals;
	unsigned int run[WR_DCS_CODES][2];
	unsigned char agree[WR_DCS_CODES][2];   /* of the last evaluation; [][0]: as sent, [][1]: inverted */
};
/* include/webradio_amd.h's rule (wr_dcs_push_rows) on `nrows` rows of `nframes` <= 2^28 floats, `row_stride` floats apart: row r
 * goes into rows[r]; words[ncodes] are the bank's 23-bit code words, `first_frame` is the clock in front of the push.  As
 * many launches as the rows' rings ask for */
hipError_t wrk_dcs_push(hipStream_t st, const float *audio, size_t row_stride, size_t nrows, size_t nframes, WrDcsRow *rows,
                        const unsigned int *words, unsigned int ncodes, unsigned int step, unsigned long long first_frame,
                        unsigned int max_errors);

/* ---- resampler (wr_resamp.hip) ---- */
/* what a push is, besides its rows: the bank's ratio and taps, the clock before it (nmod = N mod M) and the two history
 * sets [rows][P - 1] -- read from hist_old, written (for the `nrows` rows of the push) to hist_new */
struct WrResampPush {
	const float *taps;                 /* device, [L][P]; 16-byte aligned */
	unsigned int L, M, P, nmod;
	const float *hist_old;
	float       *hist_new;
};
/* the output frames a push of `nframes` yields at clock `nmod`: ceil((nmod + nframes) L / M) - ceil(nmod L / M) */
unsigned long long wrk_resamp_out_frames(unsigned int L, unsigned int M, unsigned int nmod, unsigned long long nframes);
/* include/webradio_amd.h's rule (wr_resamp_push_rows) on `nrows` rows of `nframes` floats, `row_stride` floats apart: row r
 * yields wrk_resamp_out_frames() frames at out + r * out_stride */
hipError_t wrk_resamp_push(hipStream_t st, const float *in, size_t row_stride, size_t nrows, size_t nframes, const WrResampPush &p,
                           float *out, size_t out_stride);

/* ---- voice bank (wr_voice.hip) ---- */
/* what a push is, besides its rows: the bank's filters of T taps each, the rows' control words (bits 0-7: the filter, bit 8:
 * mute) and the two history sets [rows][T - 1] -- read from hist_old, written (for the `nrows` rows of the push) to hist_new */
struct WrVoicePush {
	const float *taps;                 /* device, [nfilt][T]; 16-byte aligned */
	unsigned int T;
	const unsigned int *ctl;           /* device, [rows] */
	const float *hist_old;
	float       *hist_new;
};
/* include/webradio_amd.h's rule (wr_voice_push_rows) on `nrows` rows of `nframes` floats, `row_stride` floats apart: row r
 * yields `nframes` frames at out + r * out_stride */
hipError_t wrk_voice_push(hipStream_t st, const float *in, size_t row_stride, size_t nrows, size_t nframes, const WrVoicePush &p,
                          float *out, size_t out_stride);

hipError_t wrk_bins_to_db(hipStream_t st, const float *bins, unsigned int n, float *db);
hipError_t wrk_waterfall_row(hipStream_t st, const float *bins, unsigned int n, unsigned int width, int hold,
                             float *db_row, uint8_t *palette);

#endif /* WR_INTERNAL_H_ */
