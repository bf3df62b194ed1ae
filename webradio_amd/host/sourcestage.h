/*
 * sourcestage.h -- the GPUs of the process, and how a DspSource's current block gets onto one of them.
 *
 * Every block below one DspSource shares that source's GPU, and the source's block is brought there once per block for
 * all of them: the SpectrumSink and the tuner batch (gpubatch.h) would otherwise each push the same 32 MB over PCIe.
 * The block goes whole (stagedBlock), only its tail (stagedTail), or -- for the tuner batch alone -- only the frames
 * under the receivers' taps or in equal parts; as the RTL-SDR bytes where the source still holds them, out of
 * page-locked memory where the source's vectors can be page-locked.
 */
#ifndef WRHOST_SOURCESTAGE_H_
#define WRHOST_SOURCESTAGE_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dspblock.h"
#include "webradio_amd.h"

namespace wrhost {

/* an unsigned environment switch (any base strtoul takes), `fallback` where it is unset or empty */
unsigned int envUnsigned(const char *name, unsigned int fallback);

/* process-wide device contexts, one per GPU, opened on first use */
wr_dev *device(int index);
int deviceCount();
/* the device a block should use.  Every block below one DspSource shares that source's GPU:
 * the n-th source of the process that asks takes GPU n mod count (tuners shard one per GPU),
 * unless WEBRADIO_DEVICE pins all of them.  Blocks not below a source use WEBRADIO_DEVICE / 0. */
wr_dev *deviceFor(const DspBlock *block);
/* the DspSource at the top of `block`'s chain of producers, or NULL */
DspSource *rootSource(const DspBlock *block);
/* Device copy of the source's current block, uploaded once per source block and shared by
 * every GPU consumer of that source.  Returns NULL if `host` is not that source's current
 * output vector or the upload failed. */
const float *stagedBlock(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out);
/* false while the root source of `block` left its host vector unfilled for the current block (a byte-format
 * source all of whose consumers read on the device): a device path that fails must then fail loudly */
bool hostBlockValid(const DspBlock *block);
/* For a consumer that reads only the END of the source's block (the SpectrumSink: the most recent complete frame and what
 * follows it): the block's device address with at least its last `tail_frames` frames staged -- the whole staged block
 * where somebody staged it, else just that tail, brought over by the sparse staging kernel (a block whose receivers all
 * read it through sparse windows never crosses PCIe whole).  NULL: not fed straight from a source, or it cannot be done
 * (the caller falls back to stagedBlock). */
const float *stagedTail(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out, size_t tail_frames);

/* WEBRADIO_TRACE=1: what the tuner batches did, in order -- 'S' a block submitted (enqueued, nothing
 * waited for), 'A' audio taken from the pinned ring that was already there, 'W' audio that had to
 * be waited for.  (source, kind) pairs; tests read it to see that the front ends of a Radio have
 * their blocks in flight at the same time. */
struct TraceEvent { const void *source; char kind; };
const std::vector<TraceEvent> &trace();
void traceClear();
bool traceOn();
void traceAdd(const void *source, char kind);

/* a resizable device buffer */
struct DevBuf {
	DevBuf() : dev(NULL), ptr(NULL), bytes(0) {}
	~DevBuf() { release(); }
	bool reserve(wr_dev *d, size_t nbytes);
	void release();
	wr_dev *dev;
	void *ptr;
	size_t bytes;
};

/* ---- for the tuner batch (TunerBatch::submitOnce), which alone knows how its receivers read the block ---- */

/* the whole staged block if some consumer of the source has staged it this block already, else NULL: stages nothing */
const float *stagedBlockIfPresent(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out);
/* Sparse staging of the source's current block (wr_stage_windows_from_host): of a block whose every receiver decimates by
 * `period` through a channel filter of `length` taps only the frames under the taps -- 64 of every 400 at BASELINE config 2 --
 * and the tail cross PCIe, read by a kernel on the device's own stream, in order with the tuner's launches behind it; there
 * is no transfer to wait for and no second stream to hand over from.  period = 0: the tail alone (a SpectrumSink's frame).
 * Returns the address the WHOLE block would have on the device (the frames not staged keep what the buffer held), or NULL when
 * this block cannot be staged that way (host memory that cannot be page-locked, windows too long for the kernel): the caller
 * stages the whole block. */
const float *stagedSparse(const DspBlock *consumer, const vector<sample_t> &host, wr_dev **dev_out, unsigned int period,
                          unsigned int length, size_t tail);
/* The source's current block staged in `pieces` equal parts, part `p` (0, 1, ... in order) now: part p crosses PCIe on the
 * upload stream -- as bytes where the source still holds them (RawU8Block), converted on the device -- while the caller has
 * the parts before it worked on.  Returns the device address of the part inside the staged block, which after the last
 * part is the same staged block stagedBlock() makes in one piece (the SpectrumSink then finds it there).  NULL: this block
 * cannot be staged in parts (host memory that cannot be page-locked, no memory): before part 0 nothing has happened and the
 * caller takes the one-piece path. */
const float *stagePiece(DspSource *src, wr_dev *dev, const vector<sample_t> &host, unsigned int pieces, unsigned int p);
/* the source's current block of `floats` floats in the RTL-SDR byte format, if the source still holds it that way
 * (RawU8Block), else NULL.  Whether the bytes are USED is the caller's decision (WEBRADIO_NO_U8_STAGING) */
const uint8_t *rawBytesOf(const DspSource *src, size_t floats);

} // namespace wrhost

#endif /* WRHOST_SOURCESTAGE_H_ */
