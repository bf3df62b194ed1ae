/*
 * sourcestage.cxx -- see sourcestage.h.  The copies and conversions themselves happen behind the C ABI; this file
 * decides which of them brings a source's block to its GPU, and keeps the page locks and device buffers they need.
 */
#include "sourcestage.h"

#include <stdlib.h>

#include <mutex>

#include "debug.h"
#include "filetuner.h"
#include "gpubatch.h"

namespace wrhost {

namespace {
std::mutex g_devLock;
std::vector<wr_dev *> g_devs;
int g_sources = 0;              /* sources that have been given a GPU so far */

std::vector<TraceEvent> g_trace;
std::mutex g_traceLock;
}

unsigned int envUnsigned(const char *name, unsigned int fallback)
{
	const char *v = getenv(name);
	return (v && *v) ? (unsigned int)strtoul(v, NULL, 0) : fallback;
}

bool traceOn()
{
	static const bool on = envUnsigned("WEBRADIO_TRACE", 0) != 0;
	return on;
}

void traceAdd(const void *src, char kind)
{
	if (!traceOn())
		return;
	std::lock_guard<std::mutex> g(g_traceLock);
	TraceEvent e = { src, kind };
	g_trace.push_back(e);
}

const std::vector<TraceEvent> &trace() { return g_trace; }
void traceClear()
{
	std::lock_guard<std::mutex> g(g_traceLock);
	g_trace.clear();
}

int deviceCount()
{
	int n = 0;
	if (wr_device_count(&n) != WR_OK)
		return 0;
	return n;
}

wr_dev *device(int index)
{
	std::lock_guard<std::mutex> g(g_devLock);
	if (index < 0)
		return NULL;
	if ((size_t)index >= g_devs.size())
		g_devs.resize(index + 1, NULL);
	if (!g_devs[index]) {
		wr_dev *d = NULL;
		if (wr_dev_open(&d, index, NULL) != WR_OK) {
			/* no CPU path: the caller's init()/process() reports failure */
			LOG_ERROR("GPU device %d unavailable: %s\n", index, wr_last_error());
			return NULL;
		}
		g_devs[index] = d;
	}
	return g_devs[index];
}

DspSource *rootSource(const DspBlock *block)
{
	const DspBlock *b = block;
	while (b && b->_producer)
		b = b->_producer;
	return const_cast<DspSource *>(dynamic_cast<const DspSource *>(b));
}

bool hostBlockValid(const DspBlock *block)
{
	DspSource *src = rootSource(block);
	return !src || src->hostBlockValid();
}

bool DevBuf::reserve(wr_dev *d, size_t nbytes)
{
	if (dev == d && bytes >= nbytes && ptr)
		return true;
	release();
	if (!d || wr_dev_malloc(d, nbytes ? nbytes : 4, &ptr) != WR_OK) {
		ptr = NULL;
		return false;
	}
	dev = d;
	bytes = nbytes;
	return true;
}

void DevBuf::release()
{
	if (ptr && dev)
		wr_dev_free(dev, ptr);
	ptr = NULL;
	bytes = 0;
	dev = NULL;
}

/* the device copy of a source's current block, and the host buffers it has been uploaded from:
 * sources hand out the same one or two vectors block after block (RtlSdrTuner swaps two,
 * rtlsdrtuner.cxx:280), so they are page-locked once and the copy is a DMA nobody waits for */
struct SourceStage {
	DevBuf buf;
	DevBuf buf2;                /* a float source's blocks alternate between `buf` and `buf2`: block b + 1 crosses PCIe on the
	                               upload stream while block b is being worked on (wr_dev_upload_ahead) */
	bool second;
	DevBuf raw;                 /* the block as the source holds it in the RTL-SDR byte format (RawU8Block), on the device */
	unsigned long epoch;
	const void *host;
	size_t floats;
	wr_dev *dev;
	struct Pinned { void *ptr; size_t bytes; };
	std::vector<Pinned> pinned;
	const float *cur;           /* the staged block: in `buf`, or `buf2` */
	bool rawStaged;             /* the block now staged came from the source's raw bytes: its float vector was not read */
	/* sparse staging (stagedSparse / stagedTail): of the source's block of `sparseEpoch` only the windows
	 * [k * sparsePeriod - (sparseLen - 1), k * sparsePeriod] and the last `sparseTail` frames lie in `buf` */
	unsigned long sparseEpoch;
	unsigned int sparsePeriod, sparseLen;
	size_t sparseTail;
	size_t tailWanted;          /* the longest tail a consumer has asked for so far (a SpectrumSink: its frame + hop) */
	SourceStage() : second(false), epoch(0), host(NULL), floats(0), dev(NULL), cur(NULL), rawStaged(false), sparseEpoch(0),
	                sparsePeriod(0), sparseLen(0), sparseTail(0), tailWanted(0) {}
	~SourceStage() { unpin(); }
	/* is the WHOLE of the source's current block, handed out in `h`, staged already? */
	bool holdsWhole(const DspSource *src, const vector<sample_t> &h) const {
		return epoch == src->epoch() && host == h.data() && floats == h.size();
	}
	/* ... it is now (or, `whole` false, some of it is: no consumer may take what is staged for the whole block) */
	void nowHolds(const DspSource *src, const vector<sample_t> &h, bool whole) {
		epoch = whole ? src->epoch() : 0;
		host = h.data();
		floats = h.size();
	}
	/* the page locks must go before the memory does: freed but still registered, it is handed out
	 * again by the allocator and a later copy out of it fails ("invalid argument") */
	void unpin() {
		if (dev)
			wr_dev_wait_uploads(dev);
		for (size_t n = 0; n < pinned.size(); n++)
			wr_dev_host_unregister(dev, pinned[n].ptr);
		pinned.clear();
		epoch = 0;
		host = NULL;
	}
	bool pin(wr_dev *d, const void *p, size_t bytes) {
		for (size_t n = 0; n < pinned.size(); n++)
			if (pinned[n].ptr == p && pinned[n].bytes >= bytes)
				return true;
		if (envUnsigned("WEBRADIO_NO_PINNING", 0))
			return false;
		/* Small blocks are not page-locked: the allocator serves them from the heap, where a registered range shares
		 * its first and last page with its neighbours and its address is soon handed out again -- and on this ROCm a
		 * registered range that overlaps memory the runtime page-locks on the fly (the destination of any copy into
		 * pageable memory) can abort the process (r04: profiles/r04_abort_hunt.txt).  Large vectors get a mapping of
		 * their own from the allocator; small ones are copied through the runtime's staging buffers, which at their
		 * size costs nothing that matters. */
		static const size_t minBytes = envUnsigned("WEBRADIO_PIN_MIN_BYTES", 1u << 20);
		if (bytes < minBytes)
			return false;
		/* ... and of the large ones only those that start where a mapping of their own starts: glibc hands out a
		 * request above its mmap threshold as a private mapping with the user pointer 16 bytes into its first page
		 * (an aligned_alloc / mmap / hipHostMalloc'ed buffer starts ON a page); once the threshold has grown -- it
		 * follows the largest mapped block freed so far, up to 32 MB -- even megabytes come from the heap, in the
		 * middle of a page somebody else also lives on.  WEBRADIO_PIN_ANY=1 lifts the check. */
		static const bool pinAny = envUnsigned("WEBRADIO_PIN_ANY", 0) != 0 || minBytes == 0;
		if (!pinAny && ((uintptr_t)p & 4095u) > 64u)
			return false;
		for (size_t n = 0; n < pinned.size(); n++)
			if (pinned[n].ptr == p) {                      /* same address, grown: register afresh */
				wr_dev_wait_uploads(d);                    /* (a copy out of it may still be in flight) */
				wr_dev_host_unregister(d, pinned[n].ptr);
				pinned.erase(pinned.begin() + n);
				break;
			}
		if (pinned.size() >= 8) {                          /* (RtlSdrTuner rotates five vectors: its ring of N_BUFFERS = 4,
		                                                      rtlsdrtuner.cxx:33-34, and the one handed out)
		                                                      a source that allocates per block: give up on the oldest */
			wr_dev_wait_uploads(d);
			wr_dev_host_unregister(d, pinned[0].ptr);
			pinned.erase(pinned.begin());
		}
		if (wr_dev_host_register(d, const_cast<void *>(p), bytes) != WR_OK)
			return false;
		Pinned e = { const_cast<void *>(p), bytes };
		pinned.push_back(e);
		dev = d;
		return true;
	}
};

static void beforeSourceRun(DspSource *src);
static void beforeSourceStop(DspSource *src);

/* a source's GPU resources go with it (DspSource's destructor).  The tuner batch is one of them: this is the one call
 * from staging back to the batch */
static void releaseSource(DspSource *src)
{
	delete static_cast<SourceStage *>(src->gpuStage());
	src->setGpuStage(NULL);
	TunerBatch::destroyFor(src);
}

/* the source's stage; `create`: made now if the source has none, with the hooks that keep it safe */
static SourceStage *stageOf(DspSource *src, bool create)
{
	SourceStage *st = static_cast<SourceStage *>(src->gpuStage());
	if (!st && create) {
		st = new SourceStage();
		src->setGpuStage(st);
		src->setGpuCleanup(releaseSource);
		src->setGpuBeforeRun(beforeSourceRun);
		src->setGpuBeforeStop(beforeSourceStop);
	}
	return st;
}

/* top of DspSource::stop(): the block vector is about to be released (dspblock.cxx:153-167) */
static void beforeSourceStop(DspSource *src)
{
	SourceStage *st = stageOf(src, false);
	if (st)
		st->unpin();
}

/* top of DspSource::run(): the source is about to refill its block vector */
static void beforeSourceRun(DspSource *src)
{
	SourceStage *st = stageOf(src, false);
	if (!st || !st->dev)
		return;
	/* a source that alternates between raw buffers (RawU8Block::rawU8Buffers) may refill one while the transfer out
	 * of the other is still in flight: the host then runs a block ahead of the GPU instead of in step with it */
	unsigned int inflight = 0;
	if (st->rawStaged) {
		const RawU8Block *raw = dynamic_cast<const RawU8Block *>(src);
		const unsigned int nbuf = raw ? raw->rawU8Buffers() : 1u;
		inflight = nbuf > 1u ? (nbuf - 1u > 3u ? 3u : nbuf - 1u) : 0u;
	}
	wr_dev_wait_uploads_but(st->dev, inflight);
}

wr_dev *deviceFor(const DspBlock *block)
{
	DspSource *src = rootSource(block);
	if (!src)
		return device((int)envUnsigned("WEBRADIO_DEVICE", 0));
	if (src->gpuIndex() < 0) {
		int count = deviceCount();
		if (count <= 0) {
			LOG_ERROR("no GPU: %s\n", wr_last_error());
			return NULL;
		}
		std::lock_guard<std::mutex> g(g_devLock);
		int index = getenv("WEBRADIO_DEVICE") ? (int)envUnsigned("WEBRADIO_DEVICE", 0) : (g_sources % count);
		g_sources++;
		src->setGpuIndex(index);
		src->setGpuCleanup(releaseSource);
	}
	return device(src->gpuIndex());
}

static std::mutex g_stageLock;

const uint8_t *rawBytesOf(const DspSource *src, size_t floats)
{
	const RawU8Block *raw = dynamic_cast<const RawU8Block *>(src);
	size_t frames = 0;
	const uint8_t *bytes = raw ? raw->rawU8(&frames) : NULL;
	return (bytes && frames * 2 == floats) ? bytes : NULL;
}

/* What every staging entry begins with: the source that feeds `consumer` the vector `host` as its current block, and the
 * source's GPU in `*dev`.  NULL: not fed straight from a source (the caller uploads itself), or no GPU */
static DspSource *sourceFeeding(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev)
{
	DspSource *src = rootSource(consumer);
	if (!src || host.empty() || host.data() != src->currentBlock().data())
		return NULL;
	*dev = deviceFor(consumer);
	return *dev ? src : NULL;
}

/* ... and ends with: the block's device address, with the device it lies on where there is one */
static const float *handOut(const float *block, wr_dev *dev, wr_dev **dev_out)
{
	if (block && dev_out)
		*dev_out = dev;
	return block;
}

/* a source whose block already lies on `dev` (DeviceBlock): where */
static const float *residentBlock(const DspSource *src, wr_dev *dev, size_t floats)
{
	const DeviceBlock *db = dynamic_cast<const DeviceBlock *>(src);
	if (!db)
		return NULL;
	wr_dev *bd = NULL;
	size_t frames = 0;
	const float *p = db->deviceBlock(&bd, &frames);
	return (p && bd == dev && frames * 2 == floats) ? p : NULL;
}

const float *stagePiece(DspSource *src, wr_dev *dev, const vector<sample_t> &host, unsigned int pieces, unsigned int p)
{
	std::lock_guard<std::mutex> g(g_stageLock);
	SourceStage *st = stageOf(src, true);
	const size_t bytes = host.size() * sizeof(float);
	const uint8_t *rawBytes = rawBytesOf(src, host.size());
	const bool raw = rawBytes && !envUnsigned("WEBRADIO_NO_U8_STAGING", 0);
	if (p == 0) {
		if (st->holdsWhole(src, host))
			return NULL;                                /* somebody staged the whole block already */
		if (!raw && !src->hostBlockValid())
			return NULL;
		if (!(raw ? st->pin(dev, rawBytes, host.size()) : st->pin(dev, host.data(), bytes)))
			return NULL;
		st->dev = dev;
		if (!raw)
			st->second = !st->second;                   /* float blocks alternate between two device copies (see stageWhole) */
		DevBuf &dst = (!raw && st->second) ? st->buf2 : st->buf;
		if (!dst.reserve(dev, bytes))
			return NULL;
		st->cur = (const float *)dst.ptr;
		st->rawStaged = raw;
		st->epoch = 0;                                  /* not complete until the last part is on its way */
	}
	const size_t part = host.size() / pieces, off = part * p;      /* floats */
	float *dstp = const_cast<float *>(st->cur) + off;
	const int rc = raw ? wr_u8_to_f32_from_host(dev, rawBytes + off, dstp, part)
	                   : wr_dev_upload_ahead(dev, dstp, host.data() + off, part * sizeof(float));
	if (rc != WR_OK) {
		LOG_ERROR("staging part %u of %u of the source block failed: %s\n", p, pieces, wr_last_error());
		return NULL;
	}
	if (p + 1 == pieces)
		st->nowHolds(src, host, true);
	return dstp;
}

static bool sparseEnabled()
{
	static const bool on = envUnsigned("WEBRADIO_SPARSE", 1) != 0;
	return on;
}

/* stagedSparse, once it is known that the block has to come out of host memory */
static const float *stageSparse(DspSource *src, wr_dev *dev, const vector<sample_t> &host, unsigned int period, unsigned int length,
                                size_t tail)
{
	std::lock_guard<std::mutex> g(g_stageLock);
	SourceStage *st = stageOf(src, true);
	const size_t nframes = host.size() / 2;
	if (tail > nframes)
		tail = nframes;
	if (!period && tail > st->tailWanted)
		st->tailWanted = tail;                          /* the next block's window pass brings it along */
	if (st->holdsWhole(src, host) && st->dev == dev)
		return st->cur;                                 /* the whole block is there already */
	const bool have = st->sparseEpoch == src->epoch() && st->host == host.data() && st->floats == host.size() && st->dev == dev;
	if (have && (!period || (st->sparsePeriod == period && st->sparseLen == length)) && st->sparseTail >= tail)
		return st->cur;
	if (have && period && st->sparsePeriod)
		return NULL;                                    /* two consumers with different windows: the whole block then */
	const uint8_t *rawBytes = rawBytesOf(src, host.size());
	const bool raw = rawBytes && !envUnsigned("WEBRADIO_NO_U8_STAGING", 0);
	if (!raw && !src->hostBlockValid())
		return NULL;
	const void *from = raw ? (const void *)rawBytes : (const void *)host.data();
	const size_t bytes = host.size() * sizeof(float);
	if ((uintptr_t)from & 15u)
		return NULL;
	if (!st->pin(dev, from, raw ? host.size() : bytes) || !st->buf.reserve(dev, bytes))
		return NULL;
	if (period && st->tailWanted > tail)
		tail = st->tailWanted > nframes ? nframes : st->tailWanted;
	if (wr_stage_windows_from_host(dev, from, raw ? 1 : 0, (float *)st->buf.ptr, nframes, period ? period : (unsigned int)nframes + 1u,
	                               period ? length : 1u, tail) != WR_OK) {
		LOG_ERROR("sparse staging of the source block failed: %s\n", wr_last_error());
		return NULL;
	}
	st->dev = dev;
	st->nowHolds(src, host, false);
	st->cur = (const float *)st->buf.ptr;
	st->rawStaged = raw;
	if (!have || period) {
		st->sparsePeriod = period;
		st->sparseLen = period ? length : 0;
	}
	st->sparseTail = (have && st->sparseTail > tail) ? st->sparseTail : tail;
	st->sparseEpoch = src->epoch();
	return st->cur;
}

const float *stagedSparse(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out, unsigned int period,
                          unsigned int length, size_t tail)
{
	wr_dev *dev = NULL;
	DspSource *src = sparseEnabled() ? sourceFeeding(consumer, host, &dev) : NULL;
	if (!src)
		return NULL;
	const float *block = residentBlock(src, dev, host.size());      /* nothing to stage: the source produced it in device memory */
	if (!block)
		block = stageSparse(src, dev, host, period, length, tail);
	return handOut(block, dev, dev_out);
}

const float *stagedTail(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out, size_t tail_frames)
{
	return stagedSparse(consumer, host, dev_out, 0, 0, tail_frames);
}

/* the whole block out of host memory into `st`, for every consumer of the source */
static const float *stageWhole(SourceStage *st, DspSource *src, wr_dev *dev, const vector<sample_t> &host)
{
	const size_t bytes = host.size() * sizeof(float);
	st->dev = dev;
	/* A source that still holds the block in the RTL-SDR byte format (FileTuner; what RtlSdrTuner::dataReady
	 * receives, rtlsdrtuner.cxx:86-117): ship the BYTES -- a quarter of the float block over PCIe -- and
	 * convert on the device with the reference's rule (u8 - 128) / 128 (rtlsdrtuner.cxx:106: exact in
	 * float, so the staged block is the float block bit for bit).  Such a source need not even fill its
	 * float vector when every consumer reads the block on the device (DspBlock::readsSourceOnDevice). */
	const uint8_t *rawBytes = rawBytesOf(src, host.size());
	if (rawBytes && !envUnsigned("WEBRADIO_NO_U8_STAGING", 0)) {
		const bool pinned = st->pin(dev, rawBytes, host.size());
		/* page-locked: the bytes cross PCIe as a DMA copy on the library's upload stream, beside the kernels of
		 * the block before, and are converted on the device (wr_u8_to_f32_from_host: nothing the host waits
		 * for); else a staged copy and the kernel on the device copy */
		DevBuf &dst = st->buf;
		if (!dst.reserve(dev, bytes) ||
		    (pinned ? wr_u8_to_f32_from_host(dev, rawBytes, (float *)dst.ptr, host.size())
		            : (!st->raw.reserve(dev, host.size()) ||
		               wr_dev_upload(dev, st->raw.ptr, rawBytes, host.size()) != WR_OK)
		                  ? WR_ERR_HIP
		                  : wr_u8_to_f32(dev, (const uint8_t *)st->raw.ptr, (float *)dst.ptr, host.size())) != WR_OK) {
			LOG_ERROR("staging the source block (byte format) failed: %s\n", wr_last_error());
			return NULL;
		}
		st->nowHolds(src, host, true);
		st->rawStaged = pinned;
		st->cur = (const float *)dst.ptr;
		return st->cur;
	}
	st->rawStaged = false;
	st->cur = NULL;
	/* out of page-locked memory the copy is enqueued and the graph walk goes on beside it; the
	 * source's next run() waits for it before it touches the vector again (beforeSourceRun) */
	const bool pinned = st->pin(dev, host.data(), bytes);
	/* page-locked: on the upload stream, into the device copy the LAST block was not staged in -- the 32 MB of block
	 * b + 1 cross PCIe while the kernels of block b run (the source's next run() still waits for the copy before it
	 * touches the vector again: a float source refills the vector it swapped out at once, rtlsdrtuner.cxx:265-285) */
	if (pinned)
		st->second = !st->second;
	DevBuf &dst = (pinned && st->second) ? st->buf2 : st->buf;
	if (!dst.reserve(dev, bytes) ||
	    (pinned ? wr_dev_upload_ahead(dev, dst.ptr, host.data(), bytes)
	            : wr_dev_upload(dev, dst.ptr, host.data(), bytes)) != WR_OK) {
		LOG_ERROR("staging the source block failed: %s\n", wr_last_error());
		return NULL;
	}
	st->nowHolds(src, host, true);
	st->cur = (const float *)dst.ptr;
	return st->cur;
}

/* the whole block on the device: where the source put it, where a consumer staged it this block, or -- `stage` -- staged now */
static const float *wholeBlock(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out, bool stage)
{
	wr_dev *dev = NULL;
	DspSource *src = sourceFeeding(consumer, host, &dev);
	if (!src)
		return NULL;
	const float *block = residentBlock(src, dev, host.size());
	if (!block) {
		std::lock_guard<std::mutex> g(g_stageLock);
		SourceStage *st = stageOf(src, stage);
		if (st && st->holdsWhole(src, host))
			block = st->cur;
		else if (stage)
			block = stageWhole(st, src, dev, host);
	}
	return handOut(block, dev, dev_out);
}

const float *stagedBlock(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out)
{
	return wholeBlock(consumer, host, dev_out, true);
}

const float *stagedBlockIfPresent(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out)
{
	return wholeBlock(consumer, host, dev_out, false);
}

} // namespace wrhost
