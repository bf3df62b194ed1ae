/*
 * wr_capi_internal.h -- what the translation units of the extern "C" boundary (wr_dev.hip, wr_tuner.hip,
 * wr_tuner_submit.hip, wr_tuner_read.hip, wr_tuner_stream.hip, wr_tuner_ring.hip, wr_spectrum.hip, wr_banks.hip) share: the
 * objects behind the handles, the error macros, and ONE declaration of every helper that crosses a file boundary (the wrc_
 * names, as in wr_internal.h).  Included by those files only.
 */
#ifndef WR_CAPI_INTERNAL_H
#define WR_CAPI_INTERNAL_H

#include "wr_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <vector>

#define HIP_TRY(expr)                                                                    \
	do {                                                                                 \
		hipError_t e_ = (expr);                                                          \
		if (e_ != hipSuccess)                                                            \
			return wrc_fail(WR_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
			                __FILE__, __LINE__);                                         \
	} while (0)

/* ------------------------------------------------------------------ structs -- */

#define WR_UPLOAD_RING 4

struct wr_dev {
	int device;
	hipStream_t stream;
	bool own_stream;
	int num_cus;
	float *table;              /* [65536] reference sine table */
	float *table_turn;         /* [65536] correctly rounded sin(2 pi i / 65536): WR_NCO_ROTATE's turns */
	float *turn_host;          /* the same table on the host (per-slot turns are looked up at upload time) */
	float *hi_cs, *lo_cs;      /* [256][2] split NCO tables */
	float *scratch;            /* growable scratch */
	size_t scratch_floats;
	float *coeff;              /* [WR_FIR_MAX] staging for wr_fir_decimate */
	/* `scratch` and `coeff` are one buffer each per device, used by calls that may come from
	 * different threads (SpectrumSink::getSpectrum on HTTP threads while Radio::run() pumps,
	 * httpserver.cxx:262; two front ends on one GPU).  Work is stream-ordered once enqueued, so the
	 * lock covers a call's ENQUEUE sequence (grow -> producer kernel -> consuming copy): nobody
	 * else's kernel can land between a producer and its consumer, and nobody frees the buffer
	 * under an enqueue in progress. */
	std::mutex *scratch_lock;
	/* behind each of the last WR_UPLOAD_RING async uploads (wr_dev_upload_async, wr_u8_to_f32_from_host): upload number n
	 * (from 1) owns event n % WR_UPLOAD_RING.  `uploads_issued` - `uploads_done` are possibly still in flight. */
	hipEvent_t upload_ev[WR_UPLOAD_RING];
	std::atomic<unsigned long long> uploads_issued, uploads_done;   /* uploads and waits may come from different threads */
	std::mutex *upload_lock;
	/* wr_u8_to_f32_from_host runs on a stream of its own so that a block's bytes cross PCIe while the block before it
	 * is being worked on: up_tail[i] marks what the device's stream held when call i was made (the last readers of the
	 * buffer the call AFTER it may overwrite), up_out[i] is the buffer call i wrote */
	hipStream_t up_stream;
	hipStream_t lazy_stream = nullptr;   /* r06: the copies a SpectrumSink keeps its newest frame with beside an open streaming launch -- device to
	                                        device, i.e. copy KERNELS on this runtime, which do not start before the launch has closed: on a
	                                        stream of their own, where nothing that must not wait (the upload stream's blocks and
	                                        doorbells) can queue behind them */
	hipEvent_t up_tail[WR_UPLOAD_RING], up_done;
	void *up_out[WR_UPLOAD_RING];
	unsigned long long up_calls;
	uint8_t *up_raw[2];         /* where the DMA engine puts the bytes of a block (alternating) before the conversion kernel */
	size_t up_raw_cap[2];
	std::map<void *, size_t> *registered;   /* host ranges THIS library page-locked (wr_dev_host_register), under scratch_lock */
	/* r05: the tuner whose streaming launch (wr_tuner_set_streaming) is running on `stream` right now, or NULL.  That
	 * kernel ends when it is told to, not by itself: whoever is about to wait for the stream -- or to put work on it
	 * that must not wait for the stream's idle deadline -- closes it first (wrc_dev_stream_sync, wrc_dev_settle_stream) */
	wr_tuner *streaming = nullptr;
	unsigned long long reg_gen = 1;    /* bumped by every wr_dev_host_register / _unregister */
};
#define SCRATCH_GUARD(d) std::lock_guard<std::mutex> scratch_guard_(*(d)->scratch_lock)

struct Chan {
	bool in_use;
	int if_hz;
	unsigned int stepL;        /* phaseStep << 1 */
	unsigned int phaseL;       /* host mirror of DownConverter::phase << 1 */
	int mode;
	bool have[3];              /* [0] channel filter, [1] audio filter, [2] optional second channel filter */
	float taps[3][WR_FIR_LENGTH];
	unsigned int len1;         /* taps of the channel filter: 64 (shorter ones are zero-extended to it) or 128 / 256 */
	float taps_long[WR_FIR_FUSED_MAX];   /* ... and, when len1 > 64, the taps themselves (taps[0] is not used then) */
	unsigned int len2, len1b;  /* the same for the audio filter (stage 1) and the second channel stage (stage 2): 64, 128 or 256 */
	float taps_long2[WR_FIR_FUSED_MAX], taps_long1b[WR_FIR_FUSED_MAX];
	unsigned int decim[3];
	float gain;                /* af_gain as a factor (1 = 0 dB) */
	float squelch;             /* squelch threshold as a power (0 = open) */
	bool cs_hist_reset;        /* channel filter history (LO rows of this slot) must be zeroed */
	int group;                 /* index into wr_tuner::groups, -1 while unconfigured */
	int slot;
	float prev_iq[2];          /* only meaningful while group < 0 (parked state) */
	bool prev_dirty;           /* prev_iq must be uploaded to the slot */
	bool phase_dirty;
	bool dem_hist_reset;       /* audio filter history must be zeroed */
	/* wr_chan_set_agc: the settings as given, in dB -- wrc_group_upload derives the kernel's numbers from them for the
	 * audio rate of the group the channel sits in, so a filter change re-derives the step */
	bool agc_on;
	float agc_dbfs, agc_decay, agc_max_gain;
	bool agc_reset;            /* the AGC's state word must be set to floor */
	bool agc_used_on;          /* what the last upload gave the device (wr_chan_get_agc): AGC on, and ... */
	WrAgcPar agc_used;         /* ... these numbers */
};

struct Group {
	unsigned int d1, d2;
	unsigned int d1b = 0;      /* decimation of the second channel-filter stage, 0 = there is none */
	unsigned int l1 = WR_FIR_LENGTH;   /* taps of the group's channel filters: 64, or 128 / 256 (k_tuner_ddc_long) */
	unsigned int l2 = WR_FIR_LENGTH;   /* ... of its audio filters: 64, or 128 / 256 (k_tuner_demod + k_tuner_audio with 127 / 255 history rows) */
	unsigned int l1b = WR_FIR_LENGTH;  /* ... of its second channel stage (k_tuner_iq2) */
	int p2 = 0;                /* which iq2_hist set the next block reads */
	bool use_gain = false, use_squelch = false;
	/* some channel has its AGC on: the post stage runs with a scale of 1 and a gain of 1 in those channels' slots, does not
	 * wait for the next launch, and k_agc_rows follows it on `audio` (wr_tuner_submit.hip: submit_post) */
	bool use_agc = false;
	WrAgcPar *agc_par = nullptr;         /* [slots] */
	unsigned int *agc_state = nullptr;   /* [slots] the envelope E behind the last block */
	unsigned int slots;
	size_t k1max, k2max;
	WrGroupDev dev;
	int audio_cur = 0;         /* which member of dev.audio_set is dev.audio */
	int parity;                /* index of the current ping-pong buffers (prev_iq, dem) */
	int last_parity;           /* parity the last submit wrote its demod rows with */
	bool last_demod_kept = false; /* the last submit left its demod rows in HBM */
	/* The post stage (demodulator + audio filter) of the last block, not launched yet: it goes
	 * out with the NEXT block's DDC launch (extra workgroups of the same kernel, see
	 * k_tuner_ddc) or, when somebody needs the results first, on its own (wrc_tuner_flush). */
	bool post_pending = false;
	WrPostArgs post_args;
	/* wr_tuner_seek, lazily: the next submit's launch takes the phase in closed form (WrTunerLaunch::seeking) and reads
	 * all-zero state sets (z_hist: LO rows; z_prev; z_dem), so a seek costs no launch of its own and the post stage of the
	 * chunk before may still ride in that launch.  Anything else that touches the group's state first makes it real
	 * (seek_materialize: k_seek on the actual sets, as before r03). */
	bool seek_pending = false;
	unsigned long long seek_frame = 0;
	float *z_hist = nullptr, *z_prev = nullptr, *z_dem = nullptr;
	bool pend_direct = false;          /* that post stage writes its audio into the ring slot itself (wrc_ring_reserve) */
	unsigned long long pend_seq = 0;   /* ring bookkeeping of that block */
	size_t pend_k2 = 0;
	unsigned int pend_slots = 0;
	int sp;                    /* state set (phase, LO history) the next block reads */
	int cb;                    /* chan_iq buffer the next block writes */
	int last_cb;               /* chan_iq buffer the last submit wrote */
	std::vector<int> owner;    /* slot -> chan or -1 */
	bool dirty;                /* parameters must be uploaded before the next launch */
	bool uniform_taps;         /* each 64-slot lane group uses one channel-filter tap set */
	unsigned long long uniform_mask = 0; /* bit i: lane group i does */
	unsigned long long uniform2_mask = 0; /* bit i: the channels of lane group i share one AUDIO filter */
	unsigned long long fewsets_mask = 0; /* bit i: lane group i has at most WR_TAPSETS distinct channel filters
	                                        (the others take the per-lane-taps kernel) */
	unsigned char nsets[64] = {0};       /* how many */
	bool one_filter = false;             /* ONE channel filter for every channel of the group */
	bool long_uniform = false;           /* l1 > 64: every lane group's channels share one long filter (k_tuner_ddc_long_rot) */
	bool long_one = false;               /* ... and it is the same filter in every lane group (two lane groups per wave) */
	size_t last_k1, last_k2;
	int active;
};

struct wr_tuner {
	wr_dev *dev;
	unsigned int input_rate;
	unsigned int max_channels;
	size_t max_block_frames;
	int nco_mode;
	unsigned int keep_mask;
	std::vector<Chan> chans;
	std::vector<Group *> groups;
	float *in_stage;           /* [max_block_frames][2] for WR_HOST submits */
	int last_staging = 0;      /* how the last WR_HOST block travelled: 0 none yet, 1 copied whole, 2 staged sparsely */
	const void *probe_ptr = nullptr;   /* the last WR_HOST block found to be PAGEABLE (not asked about again while ... */
	unsigned long long probe_gen = 0;  /* ... the device's registrations stay as they were: wr_dev::reg_gen) */
	unsigned int probe_left = 0;
	float *in_hist[2];         /* [63][2] ping-pong: last 63 IQ frames of the previous block */
	int in_par;
	bool submitted;
	float audio_scale;
	unsigned long long agc_launches = 0;   /* launches of k_agc_rows so far (wr_tuner_agc_info) */
	bool profiling;
	unsigned int prof_stride;  /* 1: every submit's launch stamps its own start/stop; n > 1: one event pair
	                              around every n consecutive submits (see wr_tuner_profile) */
	unsigned int prof_tick;
	std::vector<unsigned int> ev_span;   /* launches between the events of pair i */
	/* wr_tuner_mark_launches: every launch stamps one of these on completion (its own dispatch signal, no packet of
	 * its own on the stream), so that another stream can wait for "the tuner's work so far" -- wr_ring_exchange_after */
	bool mark_launches = false;
	hipEvent_t launch_ev[4] = {nullptr, nullptr, nullptr, nullptr};
	unsigned long long launches_marked = 0;
	std::vector<hipEvent_t> ev;    /* start/stop pairs */
	size_t ev_used;                /* events recorded and not yet read */
	double prof_ms;
	unsigned int prof_n;
	/* pinned audio ring (wr_tuner_audio_ring) */
	struct RingSlot {
		float *host = nullptr;         /* pinned, [max slots][k2max] floats */
		size_t cap = 0;                /* floats */
		hipEvent_t done = nullptr;     /* the copy into this slot */
		size_t stride = 0, frames = 0;
		unsigned int slots = 0;
		unsigned long long seq = 0;
		/* a block of a streaming launch: its audio is in the slot when WrStreamCtl::done of stream number `stream_gen`
		 * has reached `stream_wait` (0: `done` is the event to wait for) */
		unsigned int stream_wait = 0;
		unsigned long long stream_gen = 0;
	};
	std::vector<RingSlot> ring;
	unsigned int ring_head = 0, ring_count = 0;    /* next slot to fill, slots queued */
	bool ring_held = false;                        /* oldest slot handed out, not yet released */
	unsigned long long ring_overruns = 0;
	unsigned long long submit_seq = 0;             /* blocks submitted so far */
	bool defer_post = true;                        /* see Group::post_pending; WR_DEFER_POST=0 turns it off */
	/* wr_tuner_set_blocks_per_launch: consecutive WR_DEVICE blocks that lie back to back in memory are
	 * held (pointer and length only) and launched as ONE block -- the bits do not depend on how the
	 * stream is cut into blocks, the fixed cost of a launch (~4.5 us at C2) is paid once per group */
	unsigned int coalesce = 1;
	const float *held_base = nullptr;
	size_t held_frames = 0, held_each = 0;
	unsigned int held_count = 0;
	std::mutex ring_lock;                          /* producer (submit) vs consumer thread */
	/* r05, wr_tuner_set_streaming: blocks in device memory go to ONE persistent launch (k_tuner_stream) through a
	 * doorbell instead of a launch each; see wr_internal.h and wrc_stream_open / wrc_stream_bell / wrc_stream_close in wr_tuner_stream.hip */
	struct Stream {
		bool enabled = false;
		bool host_bytes = false;           /* wr_tuner_set_streaming(t, 2): byte blocks out of page-locked HOST memory stream too */
		bool live = false;                 /* a launch is running and takes blocks */
		bool unchecked = false;            /* a closed launch whose outcome (WrStreamCtl::err, final_blocks) has not been read yet */
		WrStreamCtl *ctl = nullptr;        /* page-locked, mapped */
		WrStreamDesc *desc = nullptr;      /* page-locked, mapped, [WR_STREAM_MAXJ] */
		WrStreamDev *sdev = nullptr;
		float *ring = nullptr;             /* channel IQ between the DDC waves and the post stage */
		size_t ring_floats = 0;
		Group *g = nullptr;
		unsigned int count = 0;            /* blocks rung into the live (or last) launch */
		size_t nframes = 0;
		bool u8 = false;
		int parity0 = 0;
		size_t k1 = 0, k2 = 0;
		unsigned long long gen = 0;        /* launches opened so far */
		unsigned long long blocks = 0;     /* blocks streamed so far, all launches */
		std::chrono::steady_clock::time_point last_bell;
		const float *last_iq = nullptr;    /* channel IQ of the last block of the last launch (wr_chan_fetch) */
		/* r06: blocks in the RTL-SDR byte format out of PAGE-LOCKED host memory stream too (wr_tuner_submit_u8(..., WR_HOST)):
		 * the bytes cross PCIe as a DMA copy on the upload stream into one of four device buffers taken in turn, and the
		 * doorbell is rung by a 4-byte copy queued behind it (WrStreamDev::ready_up) -- the host waits for neither */
		uint8_t *raw[4] = {nullptr, nullptr, nullptr, nullptr};
		size_t raw_cap = 0;                /* bytes each */
		unsigned long long raw_next = 0;   /* submits that took a raw buffer so far */
		unsigned long long raw_gen[4] = {0, 0, 0, 0};      /* launch (gen) and block index of the buffer's last tenant */
		unsigned int raw_idx[4] = {0, 0, 0, 0};
		hipEvent_t raw_ev = nullptr;       /* behind the copy of a block that OPENS a launch: the launch waits for it */
		bool ext = false;                  /* the live launch takes such blocks (WrStreamArgs::ext) */
		bool up_pending = false;           /* doorbells of the live launch are queued on the upload stream */
		unsigned long long host_blocks = 0;    /* blocks streamed out of host memory so far */
		unsigned long long long_blocks = 0;    /* blocks of checked launches whose post stage went in long runs (WrStreamCtl::long_blocks) */
	} stream;
};

struct wr_spectrum {
	wr_dev *dev;
	unsigned int n, hop;
	unsigned int ch;           /* floats per frame: 2 (IQ) or 1 (real samples, wr_spectrum_create_real) */
	WrFftPlan plan;
	float *stage;              /* device stream buffer */
	size_t stage_cap;          /* frames */
	size_t pending;            /* frames buffered in stage, not yet consumed */
	float *bins;               /* [n][2] most recent transform */
	unsigned long frames_done;
	/* r06: a frame pushed while a streaming launch is open on the device is NOT transformed then and there (the transform
	 * would have to close the launch, every block): its frames -- from the frame's first to the block's last -- are copied
	 * into `stage` on the upload stream (the DMA engine: no wave slot needed beside the launch) and transformed when somebody
	 * asks for the spectrum (spectrum_resolve), which is what the reference's own FIXME asks for (io/spectrumsink.cxx:93-94:
	 * only the most recent frame is observable, waterfallhandler.cxx:56-61 reads it at 5 Hz) */
	bool deferred = false;
	float *keep_host = nullptr;    /* page-locked: the kept frames (from the frame's first to the block's last, padded at the front) */
	size_t keep_cap = 0;           /* frames */
	size_t def_off = 0, def_keep = 0;   /* the frame begins `def_off` frames into keep_host; `def_keep` frames from there are kept */
	size_t def_rest = 0;       /* frames behind the deferred frame's hop that belong to the NEXT frame (at stage + 2 * hop) */
	hipEvent_t def_ev = nullptr;   /* behind that copy */
	unsigned long long deferred_pushes = 0, resolves = 0;
	/* wr_spectrum_batch_avg's scratch area (wrp_spec_avg_bytes: a chunk's bins, then the carry): grows only, SPEC_AVG_BYTES at most */
	/* (wr_spectrum_rows_detect keeps a chunk's floors at its front: DETECT_FLOOR_BYTES at most) */
	float *avg = nullptr;
	size_t avg_bytes = 0;
};

/* what the four objects of wr_banks.hip, which keep something per audio row of every receiver, begin with */
struct WrRowBank {
	wr_dev *dev;
	unsigned int max_rows;
	/* wr_tuner_tones_push, wr_tuner_dcs_push, wr_tuner_resamp_push, wr_tuner_voice_push: whose submit, and which, the bank took last -- the same one is not pushed twice */
	const wr_tuner *last_tuner = nullptr;
	unsigned long long last_seq = 0;
};

struct wr_tones : WrRowBank {
	unsigned int ntones, window;
	WrTonesRow *rows;          /* device, [max_rows] */
	float *t12;                /* device, [4096]: every 16th entry of the reference sine table */
	unsigned int *steps;       /* device, [64]: the tones' phase steps, 0 beyond ntones */
};

struct wr_dcs : WrRowBank {
	unsigned int ncodes, step, max_errors;
	WrDcsRow *rows;            /* device, [max_rows] */
	unsigned int *words;       /* device, [ncodes]: the 23-bit code words */
	unsigned int zero_from = 0;        /* rows from this one on are known to be all zero */
	unsigned long long frames = 0;     /* the clock: frames since creation, a reset of every row or a seek */
};

/* the two history sets of a bank that filters its rows (wr_resamp, wr_voice): device, [max_rows][H] floats each.  A push
 * reads set `cur` and writes the other, so that no workgroup of it reads what another writes (wr_resamp.hip, wr_voice.hip) */
struct WrHistSets {
	float *set[2] = {nullptr, nullptr};
	size_t H = 0;              /* frames of history a row keeps: the filter's length less one */
	unsigned int cur = 0;
	unsigned int zero_from[2] = {0, 0};   /* rows of a set from this one on are known to hold silence */
};

struct wr_resamp : WrRowBank {
	unsigned int L, M, P;
	float *taps;               /* device, [L][P] */
	WrHistSets hist;           /* H = P - 1 */
	unsigned int nmod = 0;     /* the clock: input frames so far, mod M */
	unsigned long long frames_in = 0, frames_out = 0;
};

struct wr_voice : WrRowBank {
	unsigned int T, nfilt;
	float *taps;               /* device, [nfilt][T] */
	unsigned int *ctl;         /* device, [max_rows]: the rows' control words */
	unsigned int *ctl_host;    /* ... and the host's copy: what wr_voice_get_rows shows */
	WrHistSets hist;           /* H = T - 1 */
	unsigned long long frames = 0;
};

/* ------------------------------------------------------------------ helpers that cross files -- */

/* wr_dev.hip */
int        wrc_dev_bind(wr_dev *d);
int        wrc_dev_settle_stream(wr_dev *d);        /* closes the streaming launch that is open on the device's stream, if any */
/* (wrc_dev_stream_sync -- ... and waits for the stream -- is declared in wr_internal.h: wr_fft.hip needs it too) */
int        wrc_dev_scratch(wr_dev *d, size_t floats);
void      *wrc_host_mapped(const void *host, hipError_t *why = nullptr);
int        wrc_upload_mark_locked(wr_dev *d, hipStream_t st);
int        wrc_upload_mark(wr_dev *d, hipStream_t st);
int        wrc_dev_up_stream(wr_dev *d);
void       wrc_block_kernel_called(void);           /* one more call for wr_block_kernel_calls() to report */

/* wr_tuner.hip */
unsigned int  wrc_group_slots_used(const Group *g);
WrTunerLaunch wrc_group_launch(const wr_tuner *t, const Group *g, const float *cur, const uint8_t *cur_u8, size_t nframes);
Group        *wrc_single_group(wr_tuner *t, bool *several = nullptr);
int           wrc_post_send_pending(wr_tuner *t, Group *g, bool rode);
int           wrc_seek_materialize(wr_tuner *t, Group *g);
int           wrc_settle_held(wr_tuner *t);
int           wrc_tuner_flush(wr_tuner *t);
int           wrc_tuner_quiesce(wr_tuner *t);
int           wrc_chan_get(wr_tuner *t, int chan, Chan **c, const char *what);

/* wr_tuner_submit.hip */
int  wrc_group_upload(wr_tuner *t, Group *g);
int  wrc_tuner_launch_held(wr_tuner *t);
int  wrc_tuner_submit_now(wr_tuner *t, const void *iq, size_t nframes, int where, bool u8);
void wrc_advance_phases(wr_tuner *t, unsigned long long frames);
int  wrc_prof_pair_begin(wr_tuner *t, void **ev_start, void **ev_stop);
void wrc_prof_pair_stamped(wr_tuner *t);

/* wr_tuner_read.hip: the last submit as its readers (and the tuner pushes of wr_banks.hip) see it, in two steps (a reader's
 * own refusals go between them) */
struct WrLastSubmit {
	Group *g;                  /* the rate group read from: the tuner's one active group, or the channel's */
	unsigned int used;         /* wrc_group_slots_used(g) */
	const float *chan_iq;      /* the last block's channel IQ at the demodulator's input, [frames][g->slots][2] */
};
int wrc_last_submit_group(wr_tuner *t, const char *who, bool submitted, WrLastSubmit *v);
int wrc_last_submit_flush(wr_tuner *t, WrLastSubmit *v);

/* wr_tuner_stream.hip */
int  wrc_stream_close(wr_tuner *t);
int  wrc_stream_check(wr_tuner *t);
void wrc_stream_free(wr_tuner *t);
bool wrc_stream_follows(const wr_tuner *t, size_t nframes, int where, bool u8);
int  wrc_stream_bell(wr_tuner *t, const void *iq, bool behind_upload);
int  wrc_stream_open(wr_tuner *t, const void *iq, size_t nframes, bool u8, bool *took);
int  wrc_stream_host_u8(wr_tuner *t, const uint8_t *bytes, size_t nframes, bool *took);

/* wr_tuner_ring.hip */
float *wrc_ring_reserve(wr_tuner *t, Group *g, size_t k2, unsigned int used);
int    wrc_ring_push(wr_tuner *t, Group *g, unsigned long long seq, size_t k2, unsigned int used, bool direct);
float *wrc_stream_ring_entry(wr_tuner *t, Group *g, unsigned long long seq, size_t k2, unsigned int used, unsigned int idx);

/* (wrc_dev_settle_stream, wrc_dev_stream_sync: a streaming launch ends when it is told to, see wr_dev.hip) */
/* ... and, on a tuner's own paths, read what a launch that was closed on the way left behind (WrStreamCtl::err,
 * final_blocks) before the caller is handed results: a launch that ran into a deadline or closed itself early is an
 * error here, not stale audio with WR_OK */
/* an entry point that puts work on the device's stream (or touches the null stream) while a streaming launch is open on it:
 * close the launch first -- the work would otherwise sit behind a kernel that ends only when it is told to, or after
 * WR_STREAM_IDLE_MS of silence (include/webradio_amd.h: "calls on the same wr_dev close it first") */
#define DEV_SETTLE(d_) do { if (int rc_ = wrc_dev_settle_stream(d_)) return rc_; } while (0)
#define TUNER_SYNC_CHECKED(t_) do { HIP_TRY(wrc_dev_stream_sync((t_)->dev)); if (int rc_ = wrc_stream_check(t_)) return rc_; } while (0)

#define WR_STREAM_IDLE_MS   500           /* the launch closes itself when the doorbell has been silent this long */
#define WR_STREAM_STALE_MS  100           /* ... and the host does not ring a launch it has left alone this long: it opens a new one */
#define WR_STREAM_WAIT_MS  2000           /* deadline of every other wait inside the launch (an error) */
#define WR_STREAM_HOST_MIN_BYTES (16u << 10)   /* a host byte block streams only if it is larger than this (wrc_stream_host_u8) */

#endif
