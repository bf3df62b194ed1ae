/*
 * wr_tuner_stream.hip -- the host half of the tuner's streaming launch (wr_tuner_set_streaming): open, doorbell,
 * blocks out of page-locked host memory, close.  The device half is k_tuner_stream (wr_stream_kernel.inc); the
 * tuner itself is in wr_tuner.hip, the launch-per-block submit path in wr_tuner_submit.hip.
 */
#include "wr_capi_internal.h"

/* ------------------------------------------------------------------ the streaming launch -- */
/*
 * wr_tuner_set_streaming(tuner, 1): blocks submitted from DEVICE memory no longer cost a kernel launch each.  The
 * first one opens a persistent launch (k_tuner_stream, wr_stream_kernel.inc), every following block of the same size
 * rings its doorbell -- a descriptor and a counter in page-locked host memory -- and the launch takes it up where it
 * stands: no ramp, no tail, no kernel boundary between blocks, and a block's demodulator + audio filter start the
 * moment its last channel-IQ row is out (dsp/dspblock.cxx:169-212: a block's output leaves within its own run()).
 * Anything else that touches the tuner -- a setter, a getter, a flush, a block of another size or from host memory, a
 * wait for the device's stream through this library -- CLOSES the launch first: the host writes `stop`, the launch
 * finishes the blocks it was given, rolls the state as one launch over all of them would have, and ends.  The host's
 * own state is advanced by as many blocks at the close.  Same bits as one launch per block (tests/test_gpu_stream.py).
 *
 * Requirements, checked at the open (a submit that does not meet them goes the ordinary way): WR_NCO_ROTATE; one
 * rate group; at most 1024 channels on 64-tap channel filters, at most WR_TAPSETS distinct ones in each lane group of 64
 * channel slots; no second channel stage; an audio decimation the fused post stage has (1..6, 8, 10); an audio filter of
 * 64 or 128 taps, or of 256 up to an audio decimation of 3 (beyond it the post stage's window leaves a CU's LDS room for
 * one workgroup, and a launch needs two: DESIGN.md 3.6); blocks of at least as many channel-rate frames as the audio filter
 * has taps; whole audio frames per block; no kept demodulator rows, no seek pending, no launch marks.  A block's memory must stay untouched
 * until the NEXT block's audio is complete (the first frames of a block read the last 63 of the one before in place).
 *
 * A caller that waits for the device's stream by other means (hipStreamSynchronize on a stream it handed to
 * wr_dev_open, torch.cuda.synchronize()) should call wr_tuner_flush first: an open launch that nobody rings ends by
 * itself only after WR_STREAM_IDLE_MS.
 */

static unsigned long long *g_stream_tl = nullptr;
extern "C" int wr_debug_stream_tl(unsigned long long *out, size_t n)
{
	if (!g_stream_tl)
		return 1;
	memcpy(out, g_stream_tl, n * sizeof(unsigned long long));
	return 0;
}

/* ONE streaming launch per GPU and process: every workgroup of such a launch must be resident (they wait for one another),
 * and two of them on one device -- two wr_dev contexts, two front ends sharing a GPU -- could each hold CUs the other is
 * waiting for.  A tuner that finds the device taken submits the ordinary way.  (Other PROCESSES on the same GPU are not
 * seen from here: one process per GPU is the deployment; the launch's own deadlines end a stand-off as an error.) */
static std::mutex g_stream_mu;
static wr_tuner *g_stream_on[WR_MAX_DEVICES];

/* the four device buffers that blocks out of host memory land in */
static void stream_raw_free(wr_tuner::Stream &s)
{
	for (uint8_t *&r : s.raw) {
		(void)hipFree(r);
		r = nullptr;
	}
	s.raw_cap = 0;
}

void wrc_stream_free(wr_tuner *t)
{
	wr_tuner::Stream &s = t->stream;
	(void)hipHostFree(s.ctl);
	(void)hipHostFree(s.desc);
	(void)hipFree(s.sdev);
	(void)hipFree(s.ring);
	stream_raw_free(s);
	if (s.raw_ev)
		(void)hipEventDestroy(s.raw_ev);
	s.raw_ev = nullptr;
	s.ctl = nullptr;
	s.desc = nullptr;
	s.sdev = nullptr;
	s.ring = nullptr;
	s.ring_floats = 0;
}

/* the outcome of a closed launch, once the device's stream has been waited for */
int wrc_stream_check(wr_tuner *t)
{
	wr_tuner::Stream &s = t->stream;
	if (!s.unchecked)
		return WR_OK;
	s.unchecked = false;
	s.long_blocks += s.ctl->long_blocks;
	s.ctl->long_blocks = 0;
	if (s.ctl->err)
		return wrc_fail(WR_ERR_HIP, "streaming launch: a wait inside the launch ran into its deadline (code %u)", s.ctl->err);
	if (s.ctl->final_blocks != s.count)
		return wrc_fail(WR_ERR_STATE, "streaming launch: %u blocks rung, %u processed%s", s.count, s.ctl->final_blocks,
		                s.ctl->self_closed ? " (the launch had closed itself: the doorbell was silent too long)" : "");
	return WR_OK;
}

/* may the live launch take this block? */
bool wrc_stream_follows(const wr_tuner *t, size_t nframes, int where, bool u8)
{
	const wr_tuner::Stream &s = t->stream;
	if (!s.live || !s.enabled || where != WR_DEVICE || nframes != s.nframes || u8 != s.u8 || s.count >= WR_STREAM_MAXJ)
		return false;
	if (s.g->dirty)
		return false;
	const auto idle = std::chrono::steady_clock::now() - s.last_bell;
	return idle < std::chrono::milliseconds(WR_STREAM_STALE_MS);
}

int wrc_stream_bell(wr_tuner *t, const void *iq, bool behind_upload)
{
	wr_tuner::Stream &s = t->stream;
	const unsigned int j = s.count;
	const unsigned long long seq = t->submit_seq++;
	float *slot = wrc_stream_ring_entry(t, s.g, seq, s.k2, wrc_group_slots_used(s.g), j);
	s.desc[j].cur = (unsigned long long)(uintptr_t)iq;
	s.desc[j].audio_host = (unsigned long long)(uintptr_t)slot;
	s.desc[j].count = j + 1u;
	std::atomic_thread_fence(std::memory_order_release);      /* the descriptor before the count */
	if (behind_upload) {
		/* (r06) the block is still crossing PCIe on the upload stream: the count follows it there, into the doorbell's
		 * device-side twin -- in order with the data, nobody waits.  A stream memory operation (the command processor writes the
		 * word): a 4-byte hipMemcpyAsync is a copy KERNEL on this runtime (GPU_FORCE_BLIT_COPY_SIZE), and a kernel does not find
		 * a free wave slot with enough registers beside the launch it is supposed to ring -- measured: it ran 0.5 s later, when
		 * the launch had closed itself */
		HIP_TRY(hipStreamWriteValue32(t->dev->up_stream, &s.sdev->ready_up, j + 1u, 0));
		s.up_pending = true;
	} else {
		if (s.up_pending) {
			/* (doorbells of earlier blocks are still queued behind their copies on the upload stream: this count would overtake
			 * them -- the bell takes the larger of the two -- and ring blocks whose bytes have not landed) */
			HIP_TRY(hipStreamSynchronize(t->dev->up_stream));
			s.up_pending = false;
		}
		s.ctl->ready = j + 1u;
	}
	std::atomic_thread_fence(std::memory_order_seq_cst);
	s.count = j + 1u;
	++s.blocks;
	s.last_bell = std::chrono::steady_clock::now();
	return WR_OK;
}

int wrc_stream_open(wr_tuner *t, const void *iq, size_t nframes, bool u8, bool *took)
{
	*took = false;
	wr_tuner::Stream &s = t->stream;
	wr_dev *d = t->dev;
	if (t->nco_mode != WR_NCO_ROTATE || !t->defer_post || t->mark_launches || (t->keep_mask & (1u << WR_STAGE_DEMOD)))
		return WR_OK;
	Group *g = wrc_single_group(t);
	if (!g || g->l1 != WR_FIR_LENGTH || g->d1b || g->seek_pending || !wrk_tuner_post_supported(g->d2))
		return WR_OK;
	/* an audio filter of 64, 128 or 256 taps: 1, 2 or 4 segments of 64 in the post stage (wrk_stream_geometry says which of
	 * them a launch has room for) */
	if (g->l2 != WR_FIR_LENGTH && g->l2 != 2u * WR_FIR_LENGTH && g->l2 != 4u * WR_FIR_LENGTH)
		return WR_OK;
	const unsigned int nseg = g->l2 / WR_FIR_LENGTH;
	/* (as many channel-rate frames per block as the audio filter has taps, 64 at least: a block's post stage takes its
	 * L2 - 1 rows of history and the frame in front of them from the block before) */
	if (nframes < (size_t)g->l2 * g->d1 || nframes % ((size_t)g->d1 * g->d2) || nframes / g->d1 > 0x3FFFFFFFu)
		return WR_OK;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_launch_held(t))
		return rc;
	if (g->dirty)
		if (int rc = wrc_group_upload(t, g))
			return rc;
	if (g->use_agc)                                         /* k_agc_rows follows every block's post stage: the ordinary way */
		return WR_OK;
	const unsigned int used = wrc_group_slots_used(g), groups = used / 64u;
	if (!groups || groups > 16u)
		return WR_OK;
	/* every lane group on at most WR_TAPSETS distinct 64-tap channel filters (receiverhandler.cxx:130-137: a passband per
	 * receiver); `kmax` of them at most in one lane group.  A group with more takes the per-lane-taps kernel: the ordinary way */
	const unsigned long long used_mask = (1ull << groups) - 1ull;
	if ((g->fewsets_mask & used_mask) != used_mask)
		return WR_OK;
	const WrGroupMap map = wrp_group_map(used, 0);              /* (all of them, groups <= 16: rest = 0) */
	const unsigned int kmax = wrp_kmax(map, g->nsets);
	if (int rc = wrc_dev_settle_stream(d))                      /* another tuner's launch in this context */
		return rc;
	{
		std::lock_guard<std::mutex> lk(g_stream_mu);
		if (d->device < 0 || d->device >= WR_MAX_DEVICES || (g_stream_on[d->device] && g_stream_on[d->device] != t))
			return WR_OK;                                   /* another context's launch holds this GPU: the ordinary way */
	}
	if (s.unchecked) {
		/* the launch before this one must be over before its doorbell is reused */
		HIP_TRY(wrc_dev_stream_sync(d));
		if (int rc = wrc_stream_check(t))
			return rc;
	}
	if (g->post_pending)                                    /* the post stage of a block that went the ordinary way */
		if (int rc = wrc_tuner_flush(t))
			return rc;
	const size_t k1 = nframes / g->d1, k2 = k1 / g->d2;
	unsigned int n_ddc = 0, n_post = 0;
	HIP_TRY(wrk_stream_geometry(g->d2, groups, kmax, g->one_filter, nseg, d->num_cus, &n_ddc, &n_post));
	if (!n_ddc || !n_post)
		return WR_OK;
	/* (each on its own: an allocation that failed last time is tried again, never skipped because an earlier one stands) */
	if (!s.ctl)
		HIP_TRY(hipHostMalloc((void **)&s.ctl, sizeof(WrStreamCtl), hipHostMallocMapped | hipHostMallocCoherent));
	if (!s.desc)
		HIP_TRY(hipHostMalloc((void **)&s.desc, sizeof(WrStreamDesc) * WR_STREAM_MAXJ, hipHostMallocMapped | hipHostMallocCoherent));
	if (!s.sdev)
		HIP_TRY(hipMalloc((void **)&s.sdev, sizeof(WrStreamDev)));
	const size_t ring_floats = (size_t)WR_STREAM_RING * k1 * g->slots * 2u;
	if (ring_floats > s.ring_floats) {
		HIP_TRY(wrc_dev_stream_sync(d));
		(void)hipFree(s.ring);
		s.ring = nullptr;
		s.ring_floats = 0;
		HIP_TRY(hipMalloc((void **)&s.ring, ring_floats * sizeof(float)));
		s.ring_floats = ring_floats;
	}
	void *ctl_dev = nullptr, *desc_dev = nullptr;
	HIP_TRY(hipHostGetDevicePointer(&ctl_dev, s.ctl, 0));
	HIP_TRY(hipHostGetDevicePointer(&desc_dev, s.desc, 0));
	hipStream_t st = d->stream;

	/* the launch's view of the group: what wrc_tuner_submit_now hands k_tuner_ddc and the post stage for one block */
	const WrTunerLaunch L = wrc_group_launch(t, g, u8 ? nullptr : (const float *)iq, u8 ? (const uint8_t *)iq : nullptr, nframes);

	WrStreamArgs A;
	memset(&A, 0, sizeof(A));
	A.ctl = (WrStreamCtl *)ctl_dev;
	A.desc_host = (const WrStreamDesc *)desc_dev;
	A.sdev = s.sdev;
	A.idle_ticks = (unsigned long long)WR_STREAM_IDLE_MS * 100000ull;      /* the constant clock runs at 100 MHz */
	A.wait_ticks = (unsigned long long)WR_STREAM_WAIT_MS * 100000ull;
	A.n_ddc = n_ddc;
	A.n_post = n_post;
	if (getenv("WR_STREAM_TL") && atoi(getenv("WR_STREAM_TL"))) {      /* the timeline of a -DSTREAM_TL build */
		static unsigned long long *tlbuf = nullptr;
		if (!tlbuf)
			HIP_TRY(hipHostMalloc((void **)&tlbuf, 8192 * 8 * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent));
		memset(tlbuf, 0, 8192 * 8 * sizeof(unsigned long long));
		void *tld = nullptr;
		HIP_TRY(hipHostGetDevicePointer(&tld, tlbuf, 0));
		A.tl = (unsigned long long *)tld;
		g_stream_tl = tlbuf;
	}
	A.nframes = nframes;
	A.k1 = (unsigned int)k1;
	A.d1 = g->d1;
	A.is_u8 = u8 ? 1u : 0u;
	A.ext = s.ext ? 1u : 0u;
	A.slots = g->slots;
	A.groups = groups;
	A.gmap0 = map.gmap[0];
	A.gmap1 = map.gmap[1];
	A.kslow = wrp_kslow(g->d1, k1);
	A.hist = L.hist;
	A.hist_next = L.hist_next;
	A.phase = g->dev.phase[g->sp];
	A.step = g->dev.step;
	A.phase_next = g->dev.phase[g->sp ^ 1];
	A.hist_cs = g->dev.hist_cs[g->sp];
	A.hist_lo = g->dev.hist_lo[g->sp];
	A.hist_cs_next = g->dev.hist_cs[g->sp ^ 1];
	A.hist_lo_next = g->dev.hist_lo[g->sp ^ 1];
	A.flags = g->dev.flags;
	A.taps1 = g->dev.taps1;
	A.rot = g->dev.rot;
	A.taps1u = g->dev.taps1u;
	A.tapsel = g->dev.tapsel;
	A.table = d->table_turn;
	A.hi_cs = d->hi_cs;
	A.lo_cs = d->lo_cs;
	A.ring = s.ring;
	for (int i = 0; i < 4; ++i)
		A.audio_bufs[i] = g->dev.audio_set[(g->audio_cur + i) & 3];
	A.post = wrk_post_args(L, g->dev);                      /* (nseg, and taps2u [lane groups][L2], with it) */
	A.post.host_stride = k2;                                /* the ring's rows lie back to back (RingSlot::stride = frames) */
	A.prev_iq[0] = g->dev.prev_iq[0];
	A.prev_iq[1] = g->dev.prev_iq[1];
	A.dem[0] = g->dev.dem[0];
	A.dem[1] = g->dev.dem[1];
	A.parity0 = g->parity;
	A.kmax = kmax;
	A.one_filter = g->one_filter ? 1u : 0u;

	/* the doorbell as the launch finds it: block 0 rung */
	++s.gen;
	s.g = g;
	s.count = 0;
	s.nframes = nframes;
	s.u8 = u8;
	s.parity0 = g->parity;
	s.k1 = k1;
	s.k2 = k2;
	s.last_iq = nullptr;
	const unsigned long long seq = t->submit_seq++;
	float *slot = wrc_stream_ring_entry(t, g, seq, k2, used, 0);
	s.ctl->ready = 1;
	s.ctl->stop = 0;
	s.ctl->done = 0;
	s.ctl->final_blocks = 0;
	s.ctl->long_blocks = 0;
	s.ctl->err = 0;
	s.ctl->self_closed = 0;
	s.desc[0].cur = (unsigned long long)(uintptr_t)iq;
	s.desc[0].audio_host = (unsigned long long)(uintptr_t)slot;
	std::atomic_thread_fence(std::memory_order_seq_cst);
	/* the counters, the progress words and the doorbell's device-side copy start from zero: one fill.  (Block 0's
	 * descriptor travels in the kernel's arguments; WrStreamDev::ready stays 0 until the bell republishes a count of 2
	 * or more -- it is NOT copied from the doorbell here: that copy would run when the stream gets to it, by which time
	 * the host may have rung again, and the bell, finding the higher count already in device memory, would never bring
	 * the descriptors over that go with it) */
	if (s.ext) {
		/* A launch that takes blocks out of host memory: WrStreamDev::ready_up is NOT part of this fill.  Its doorbells are
		 * written on the UPLOAD stream, which does not wait for the device's: with small blocks the first of them could land
		 * before this fill runs, and the fill would wipe the count (the launch then never sees the block).  wrc_stream_host_u8
		 * zeroes ready_up on the upload stream instead, behind block 0's copy and ahead of raw_ev -- before every doorbell of
		 * this launch by the upload stream's order, and before the launch starts by the wait on raw_ev. */
		HIP_TRY(hipMemsetAsync(s.sdev, 0, offsetof(WrStreamDev, ready_up), st));
		const size_t after = offsetof(WrStreamDev, ready_up) + sizeof(unsigned int);
		HIP_TRY(hipMemsetAsync((char *)s.sdev + after, 0, offsetof(WrStreamDev, desc) - after, st));
	} else {
		HIP_TRY(hipMemsetAsync(s.sdev, 0, offsetof(WrStreamDev, desc), st));
	}
	A.cur0 = s.desc[0].cur;
	A.audio0 = s.desc[0].audio_host;

	void *ev0 = nullptr, *ev1 = nullptr;
	if (t->profiling && !(t->ev_used & 1))
		/* one event pair for the whole launch, stamped by the dispatch itself (none while a group's start event is open) */
		if (int rc = wrc_prof_pair_begin(t, &ev0, &ev1))
			return rc;
	HIP_TRY(wrk_tuner_stream(st, A, ev0, ev1));
	if (ev0)
		wrc_prof_pair_stamped(t);
	s.live = true;
	s.count = 1;
	++s.blocks;
	s.last_bell = std::chrono::steady_clock::now();
	d->streaming = t;
	{
		std::lock_guard<std::mutex> lk(g_stream_mu);
		g_stream_on[d->device] = t;
	}
	*took = true;
	return WR_OK;
}

/* r06: a block in the RTL-SDR byte format out of PAGE-LOCKED host memory, streamed (see wr_tuner::Stream::raw).  `*took` false:
 * not this way (pageable memory, a shape the launch cannot take, no memory) -- the caller goes the ordinary way. */
int wrc_stream_host_u8(wr_tuner *t, const uint8_t *bytes, size_t nframes, bool *took)
{
	*took = false;
	wr_tuner::Stream &s = t->stream;
	wr_dev *d = t->dev;
	if (wrc_dev_bind(d))
		return WR_ERR_HIP;
	if (!wrc_host_mapped(bytes))
		return WR_OK;                                       /* pageable: the copy would be staged by the runtime, synchronously */
	const size_t need = nframes * 2;
	/* A copy of WR_STREAM_HOST_MIN_BYTES or less is a copy KERNEL on this runtime (GPU_FORCE_BLIT_COPY_SIZE), and a kernel does
	 * not start beside the open launch (see wrc_stream_bell): the block's doorbell, queued behind its copy, would never ring and the
	 * launch would close itself with the block untaken.  Such a block goes the ordinary way. */
	if (need <= WR_STREAM_HOST_MIN_BYTES)
		return WR_OK;
	const bool follows = s.live && s.ext && wrc_stream_follows(t, nframes, WR_DEVICE, true);
	if (need > s.raw_cap) {
		if (int rc = wrc_stream_close(t))
			return rc;
		HIP_TRY(wrc_dev_stream_sync(d));
		if (d->up_stream)
			HIP_TRY(hipStreamSynchronize(d->up_stream));
		stream_raw_free(s);
		for (uint8_t *&r : s.raw)
			HIP_TRY(hipMalloc((void **)&r, need));
		s.raw_cap = need;
	}
	const unsigned int slot = (unsigned int)(s.raw_next & 3u);
	/* the buffer's last tenant and the block behind it, whose first windows reach into its tail, must be through before the copy
	 * below is queued: their audio (WrStreamCtl::done) comes behind the last read of their frames.  The tenant may be four
	 * blocks back in the live launch (a caller far ahead of the GPU), or a block of a launch that has been CLOSED but may still
	 * be running (s.unchecked: nobody has waited for the device's stream since the stop) -- the copy is on the upload stream,
	 * which does not wait for the device's, so only this wait orders the launch's last read of the buffer before the new
	 * bytes.  A closed launch ends with done == count, so the block behind the tenant is waited for only if it was rung. */
	const unsigned int through = s.raw_idx[slot] + 2u < s.count ? s.raw_idx[slot] + 2u : s.count;
	if ((s.live || s.unchecked) && s.raw_gen[slot] == s.gen && s.ctl->done < through) {
		const auto t0 = std::chrono::steady_clock::now();
		while (s.ctl->done < through && !s.ctl->err)
			if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4 * WR_STREAM_WAIT_MS))
				return wrc_fail(WR_ERR_HIP, "streaming launch: block %u did not finish", s.raw_idx[slot] + 1u);
	}
	{
		std::lock_guard<std::mutex> up_guard(*d->upload_lock);
		if (int rc = wrc_dev_up_stream(d))
			return rc;
		HIP_TRY(hipMemcpyAsync(s.raw[slot], bytes, need, hipMemcpyHostToDevice, d->up_stream));
		if (int rc = wrc_upload_mark_locked(d, d->up_stream))   /* (wr_dev_wait_uploads: the host block is free again when the copy has run) */
			return rc;
	}
	if (follows) {
		s.raw_gen[slot] = s.gen;
		s.raw_idx[slot] = s.count;
		++s.raw_next;
		++s.host_blocks;
		t->last_staging = 3;
		*took = true;
		return wrc_stream_bell(t, s.raw[slot], true);
	}
	if (int rc = wrc_stream_close(t))
		return rc;
	/* this block opens a launch (or, if it cannot, goes the ordinary way out of the device copy): either waits for the copy */
	if (!s.raw_ev)
		HIP_TRY(hipEventCreateWithFlags(&s.raw_ev, hipEventDisableTiming));
	/* the doorbell's device-side twin starts from zero for the launch this block may open (see wrc_stream_open): written on the
	 * upload stream, behind everything a launch before this one rang there and ahead of this launch's own doorbells.  (A
	 * launch that was closed and may still run ignores it: its count is final in WrStreamCtl::ready, wrc_stream_close.)  A stream
	 * memory operation, not a fill kernel: see wrc_stream_bell. */
	if (!s.sdev)
		HIP_TRY(hipMalloc((void **)&s.sdev, sizeof(WrStreamDev)));
	HIP_TRY(hipStreamWriteValue32(d->up_stream, &s.sdev->ready_up, 0u, 0));
	HIP_TRY(hipEventRecord(s.raw_ev, d->up_stream));
	HIP_TRY(hipStreamWaitEvent(d->stream, s.raw_ev, 0));
	s.ext = true;
	bool opened = false;
	if (int rc = wrc_stream_open(t, s.raw[slot], nframes, true, &opened))
		return rc;
	s.raw_gen[slot] = opened ? s.gen : 0;
	s.raw_idx[slot] = 0;
	++s.raw_next;
	*took = true;
	if (opened) {
		++s.host_blocks;
		t->last_staging = 3;
		return WR_OK;
	}
	s.ext = false;
	t->last_staging = 1;
	return wrc_tuner_submit_now(t, s.raw[slot], nframes, WR_DEVICE, true);
}

/* close the live launch: tell it that no block follows, and advance the host's picture of the tuner by the blocks
 * it was given.  Does not wait: the launch finishes them and ends, stream-ordered work queues behind it. */
int wrc_stream_close(wr_tuner *t)
{
	wr_tuner::Stream &s = t->stream;
	if (!s.live)
		return WR_OK;
	if (s.up_pending) {
		/* doorbells still queued behind their blocks on the upload stream: the count must be final before the stop */
		HIP_TRY(hipStreamSynchronize(t->dev->up_stream));
		s.ctl->ready = s.count;
		s.up_pending = false;
	}
	std::atomic_thread_fence(std::memory_order_seq_cst);
	s.ctl->stop = 1;
	std::atomic_thread_fence(std::memory_order_seq_cst);
	s.live = false;
	s.unchecked = true;
	if (t->dev->streaming == t)
		t->dev->streaming = nullptr;
	{
		std::lock_guard<std::mutex> lk(g_stream_mu);
		if (g_stream_on[t->dev->device] == t)
			g_stream_on[t->dev->device] = nullptr;
	}
	Group *g = s.g;
	const unsigned int J = s.count;
	for (Group *x : t->groups)
		if (x != g)
			x->last_k1 = x->last_k2 = 0;
	g->sp ^= 1;                        /* the launch rolls the DDC's state into the other set ONCE, behind its last block */
	g->last_parity = s.parity0;
	g->parity = s.parity0 ^ 1;         /* ... and so it does with the post stage's */
	g->last_k1 = s.k1;
	g->last_k2 = s.k2;
	g->last_demod_kept = false;
	s.last_iq = s.ring + (size_t)((J - 1u) % WR_STREAM_RING) * s.k1 * g->slots * 2u;
	/* the blocks of a stream store their audio into the group's four device arrays by turns (blocks' post stages
	 * may run side by side); the one the LAST block wrote is the group's audio from here on */
	g->audio_cur = (int)((g->audio_cur + (J - 1u)) & 3u);
	g->dev.audio = g->dev.audio_set[g->audio_cur];
	t->in_par ^= 1;
	wrc_advance_phases(t, (unsigned long long)s.nframes * J);
	t->submitted = true;
	return WR_OK;
}

extern "C" int wr_tuner_set_streaming(wr_tuner *t, int enable)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (int rc = wrc_tuner_launch_held(t))
		return rc;
	t->stream.enabled = enable != 0;
	t->stream.host_bytes = enable >= 2;
	return WR_OK;
}

extern "C" int wr_tuner_stream_info(wr_tuner *t, int *live, unsigned long long *launches, unsigned long long *blocks)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (live)
		*live = t->stream.live ? 1 : 0;
	if (launches)
		*launches = t->stream.gen;
	if (blocks)
		*blocks = t->stream.blocks;
	return WR_OK;
}

extern "C" int wr_tuner_stream_long_blocks(wr_tuner *t, unsigned long long *blocks)
{
	if (!t || !blocks)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_stream_long_blocks: bad argument");
	*blocks = t->stream.long_blocks;
	return WR_OK;
}

extern "C" int wr_tuner_stream_host_blocks(wr_tuner *t, unsigned long long *blocks)
{
	if (!t || !blocks)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_stream_host_blocks: bad argument");
	*blocks = t->stream.host_blocks;
	return WR_OK;
}
