/*
 * wr_tuner_ring.hip -- the tuner's pinned audio ring (wr_tuner_audio_ring): blocks of audio queued in page-locked
 * host memory by the submit path (wr_tuner_submit.hip) and by the streaming launch (wr_tuner_stream.hip), handed out in
 * order to a consumer thread.
 */
#include "wr_capi_internal.h"

/* the slot's page-locked buffer, grown to the group's largest block */
static hipError_t ring_slot_grow(wr_tuner::RingSlot &r, const Group *g)
{
	(void)hipHostFree(r.host);
	r.host = nullptr;
	r.cap = 0;
	const size_t want = (size_t)g->slots * g->k2max;
	const hipError_t e = hipHostMalloc((void **)&r.host, (want ? want : 1) * sizeof(float), hipHostMallocDefault);
	if (e == hipSuccess)
		r.cap = want;
	return e;
}

/* the next slot to fill is block `seq`'s (`stream_wait`: see RingSlot); under ring_lock */
static void ring_queue(wr_tuner *t, unsigned long long seq, size_t k2, unsigned int used, unsigned int stream_wait)
{
	wr_tuner::RingSlot &r = t->ring[t->ring_head];
	r.stream_wait = stream_wait;
	r.stream_gen = t->stream.gen;               /* (read only where stream_wait is set) */
	r.stride = r.frames = k2;
	r.slots = used;
	r.seq = seq;
	t->ring_head = (t->ring_head + 1) % (unsigned int)t->ring.size();
	++t->ring_count;
}

/* r04: the post stage whose arguments are being put together (a deferred one: it is launched later, riding in the next
 * block's launch or by a flush) may write its audio straight into the ring slot its block will be queued in -- the next
 * one to fill, which stays the next one until that block's own wrc_ring_push: pushes come in block order and this group is
 * the only one that pushes.  The audio is then in the ring when the launch has run; no device-to-host copy is enqueued
 * behind it (50 us for the 2 MB of a C2 block, in series with everything else of an on-time block).  Returns the slot's
 * device-side address, or NULL: no ring, several rate groups, the ring full right now (the block may still be queued by
 * copy if a slot is free by then), or page-locked memory that cannot be had. */
float *wrc_ring_reserve(wr_tuner *t, Group *g, size_t k2, unsigned int used)
{
	if (t->ring.empty())
		return nullptr;
	std::lock_guard<std::mutex> lk(t->ring_lock);
	if (wrc_single_group(t) != g || t->ring_count == t->ring.size())
		return nullptr;
	wr_tuner::RingSlot &r = t->ring[t->ring_head];
	const size_t need = (size_t)used * k2;
	if (!need)
		return nullptr;
	if (need > r.cap && ring_slot_grow(r, g) != hipSuccess) {
		(void)hipGetLastError();
		r.host = nullptr;
		return nullptr;
	}
	return (float *)wrc_host_mapped(r.host);
}

/* a ring entry for block `idx` (from 0) of the live launch: its audio is complete when WrStreamCtl::done > idx */
float *wrc_stream_ring_entry(wr_tuner *t, Group *g, unsigned long long seq, size_t k2, unsigned int used, unsigned int idx)
{
	if (t->ring.empty())
		return nullptr;
	float *mapped = wrc_ring_reserve(t, g, k2, used);
	std::lock_guard<std::mutex> lk(t->ring_lock);
	if (!mapped) {
		if (wrc_single_group(t) == g && t->ring_count == t->ring.size())
			++t->ring_overruns;                         /* io/rtlsdrtuner.cxx:100-117: the new block is dropped */
		return nullptr;
	}
	ring_queue(t, seq, k2, used, idx + 1u);
	return mapped;
}

int wrc_ring_push(wr_tuner *t, Group *g, unsigned long long seq, size_t k2, unsigned int used, bool direct)
{
	if (t->ring.empty())
		return WR_OK;
	std::lock_guard<std::mutex> lk(t->ring_lock);
	if (wrc_single_group(t) != g)
		return WR_OK;                           /* no or several rate groups: not queued (see the header) */
	if (t->ring_count == t->ring.size()) {
		++t->ring_overruns;                     /* io/rtlsdrtuner.cxx:100-117: the new block is dropped */
		return WR_OK;
	}
	wr_tuner::RingSlot &r = t->ring[t->ring_head];
	const size_t need = (size_t)used * k2;
	if (need > r.cap) {
		HIP_TRY(ring_slot_grow(r, g));
		direct = false;                         /* (cannot happen: wrc_ring_reserve sized the slot) */
	}
	hipStream_t st = t->dev->stream;
	if (need && !direct) {
		if (k2 == g->k2max)                     /* rows back to back (the usual block size): one linear copy */
			HIP_TRY(hipMemcpyAsync(r.host, g->dev.audio, need * sizeof(float), hipMemcpyDeviceToHost, st));
		else
			HIP_TRY(hipMemcpy2DAsync(r.host, k2 * sizeof(float), g->dev.audio, g->k2max * sizeof(float),
			                         k2 * sizeof(float), used, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipEventRecord(r.done, st));
	ring_queue(t, seq, k2, used, 0);
	return WR_OK;
}

extern "C" int wr_tuner_audio_ring(wr_tuner *t, unsigned int depth)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	if (depth > 1024)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_audio_ring: depth %u", depth);
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	if (int rc = wrc_settle_held(t))
		return rc;
	{
		int rc = wrc_tuner_quiesce(t);               /* no copy may be in flight into a slot we free */
		if (rc)
			return rc;
	}
	std::lock_guard<std::mutex> lk(t->ring_lock);
	if (t->ring_held)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_audio_ring: a slot is still acquired");
	for (wr_tuner::RingSlot &r : t->ring) {
		if (r.done)
			(void)hipEventDestroy(r.done);
		(void)hipHostFree(r.host);
	}
	t->ring.clear();
	t->ring.resize(depth);
	for (wr_tuner::RingSlot &r : t->ring)
		HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
	t->ring_head = t->ring_count = 0;
	t->ring_overruns = 0;
	return WR_OK;
}

extern "C" int wr_tuner_audio_ring_acquire(wr_tuner *t, const float **audio_host, size_t *chan_stride,
                                           size_t *frames, unsigned int *slots_used, unsigned long long *seq)
{
	if (!t || !audio_host || !chan_stride || !frames || !slots_used)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_audio_ring_acquire: bad argument");
	hipEvent_t ev;
	wr_tuner::RingSlot *r;
	unsigned int swait = 0;
	unsigned long long sgen = 0;
	{
		std::lock_guard<std::mutex> lk(t->ring_lock);
		if (t->ring.empty())
			return wrc_fail(WR_ERR_STATE, "wr_tuner_audio_ring_acquire: no ring (wr_tuner_audio_ring)");
		if (t->ring_held)
			return wrc_fail(WR_ERR_STATE, "wr_tuner_audio_ring_acquire: release the previous slot first");
		if (!t->ring_count)
			return wrc_fail(WR_ERR_STATE, "wr_tuner_audio_ring_acquire: nothing queued");
		const unsigned int n = (unsigned int)t->ring.size();
		r = &t->ring[(t->ring_head + n - t->ring_count) % n];
		ev = r->done;
		swait = r->stream_wait;
		sgen = r->stream_gen;
		t->ring_held = true;
	}
	/* wait outside the lock: the producer may queue further blocks meanwhile */
	hipError_t e = hipSuccess;
	if (swait) {
		/* a block of a streaming launch: the launch's post stage wrote the slot itself and counts the blocks it has
		 * finished in page-locked memory (a launch older than the tuner's current one has ended: wrc_stream_open waits) */
		const auto t0 = std::chrono::steady_clock::now();
		unsigned int spins = 0;
		while (sgen == t->stream.gen && t->stream.ctl->done < swait && !t->stream.ctl->err) {
			if ((++spins & 1023u) == 0u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(4 * WR_STREAM_WAIT_MS)) {
				std::lock_guard<std::mutex> lk(t->ring_lock);
				t->ring_held = false;
				return wrc_fail(WR_ERR_HIP, "wr_tuner_audio_ring_acquire: the streaming launch did not deliver block %u", swait - 1u);
			}
#if defined(__x86_64__)
			__builtin_ia32_pause();
#endif
		}
		std::atomic_thread_fence(std::memory_order_acquire);
		if (sgen == t->stream.gen && t->stream.ctl->err) {
			std::lock_guard<std::mutex> lk(t->ring_lock);
			t->ring_held = false;
			return wrc_fail(WR_ERR_HIP, "wr_tuner_audio_ring_acquire: the streaming launch reported error %u", t->stream.ctl->err);
		}
	} else {
		e = hipEventSynchronize(ev);        /* (looking at the event ourselves first -- hipEventQuery in a loop -- changes nothing:
		                                       what an on-time caller waits for here is the GPU, not the wake-up; r05) */
	}
	if (e != hipSuccess) {
		std::lock_guard<std::mutex> lk(t->ring_lock);
		t->ring_held = false;
		return wrc_fail(WR_ERR_HIP, "wr_tuner_audio_ring_acquire: %s", hipGetErrorString(e));
	}
	*audio_host = r->host;
	*chan_stride = r->stride;
	*frames = r->frames;
	*slots_used = r->slots;
	if (seq)
		*seq = r->seq;
	return WR_OK;
}

/* has the copy of the oldest queued block landed (would wr_tuner_audio_ring_acquire return at once)? */
extern "C" int wr_tuner_audio_ring_ready(wr_tuner *t, int *ready)
{
	if (!t || !ready)
		return wrc_fail(WR_ERR_ARG, "wr_tuner_audio_ring_ready: bad argument");
	*ready = 0;
	hipEvent_t ev;
	{
		std::lock_guard<std::mutex> lk(t->ring_lock);
		if (t->ring.empty() || !t->ring_count || t->ring_held)
			return WR_OK;
		const unsigned int n = (unsigned int)t->ring.size();
		const wr_tuner::RingSlot &r = t->ring[(t->ring_head + n - t->ring_count) % n];
		ev = r.done;
		if (r.stream_wait) {
			*ready = (r.stream_gen != t->stream.gen || t->stream.ctl->done >= r.stream_wait) ? 1 : 0;
			return WR_OK;
		}
	}
	if (wrc_dev_bind(t->dev))
		return WR_ERR_HIP;
	const hipError_t e = hipEventQuery(ev);
	if (e == hipSuccess)
		*ready = 1;
	else if (e != hipErrorNotReady)
		return wrc_fail(WR_ERR_HIP, "wr_tuner_audio_ring_ready: %s", hipGetErrorString(e));
	return WR_OK;
}

extern "C" int wr_tuner_audio_ring_release(wr_tuner *t)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	std::lock_guard<std::mutex> lk(t->ring_lock);
	if (!t->ring_held)
		return wrc_fail(WR_ERR_STATE, "wr_tuner_audio_ring_release: nothing acquired");
	t->ring_held = false;
	--t->ring_count;
	return WR_OK;
}

extern "C" int wr_tuner_audio_ring_stats(wr_tuner *t, unsigned int *queued, unsigned long long *overruns)
{
	if (!t)
		return wrc_fail(WR_ERR_ARG, "tuner is NULL");
	std::lock_guard<std::mutex> lk(t->ring_lock);
	if (queued)
		*queued = t->ring_count;
	if (overruns)
		*overruns = t->ring_overruns;
	return WR_OK;
}
