/*
 * gpubatch.h -- host glue between the DspBlock graph and the C ABI (webradio_amd.h).
 *
 * The reference walks the graph depth first, one Receiver after the other
 * (dspblock.cxx:207-209), and every block materialises its output.  The GPU wants the
 * opposite: all Receivers of a tuner in one launch sequence, and none of the full-rate
 * intermediates.  TunerBatch reconciles the two without changing the graph API:
 *
 *   - when a DownConverter that hangs directly off a DspSource is started and the blocks
 *     after it form exactly the Receiver chain of radio.cxx:68-76
 *     (DownConverter -> LowPass -> Demodulator -> LowPass), the four blocks are enrolled
 *     as one CHANNEL of the source's TunerBatch (a wr_tuner on one GPU); so is the same chain
 *     with a second LowPass in front of the demodulator (narrow channels off a fast stream);
 *   - the first enrolled DownConverter::process() of a source block ("epoch") has the tuner
 *     buffer brought to the GPU once (sourcestage.h) and submits every channel; later process() calls of enrolled
 *     blocks in the same epoch are no-ops, except the audio LowPass, which copies its
 *     channel's audio out of the batch's single device-to-host transfer;
 *   - SpectrumSinks on the last channel filter of such a chain (a panadapter per listener) do not end the fusion:
 *     they receive no samples, and getSpectrum() is served from the channel IQ the tuner keeps of its last submit --
 *     one wr_tuner_chan_spectra launch and one copy for all the sinks that ask about the same block;
 *   - blocks that are not part of such a chain run one kernel each (wr_mix,
 *     wr_fir_decimate, wr_demod) on their own host buffers.
 */
#ifndef WRHOST_GPUBATCH_H_
#define WRHOST_GPUBATCH_H_

#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "dspblock.h"
#include "sourcestage.h"
#include "webradio_amd.h"

class DownConverter;
class LowPass;
class Demodulator;
class SpectrumSink;

namespace wrhost {

/* ---- questions to the tuner batch of a block's root source ---- */

/* r06: did the tuner batch of `block`'s root source stream (a DeviceBlock source: wr_tuner_set_streaming)?  `live`: a launch is
 * open right now; `launches` / `blocks`: opened / taken so far.  false: no batch */
bool streamInfo(const DspBlock *block, bool *live, unsigned long long *launches, unsigned long long *blocks);
/* how many wr_tuner_chan_spectra calls the tuner batch of `block`'s root source has made (0: no batch) */
unsigned long long chanSpectraCalls(const DspBlock *block);
/* ... and how many wr_tuner_chan_levels calls (Demodulator::inputLevel of its enrolled receivers: one per block asked about) */
unsigned long long chanLevelCalls(const DspBlock *block);
/* For a consumer of the source's block that is NOT part of the tuner batch (the SpectrumSink, which FrontEnd connects
 * first): have the batch submit this block now, before the consumer enqueues its own work -- the receivers' launches then
 * come first on the device's stream and the audio does not wait behind the spectrum's copy and transform (the batch
 * submits once per block whoever asks first).  No batch, or not the source's current block: nothing happens. */
void submitBatchFirst(const DspBlock *consumer, const vector<sample_t> &host);

class TunerBatch;

struct Channel {
	TunerBatch *batch;
	int id;                       /* wr_tuner channel id */
	int slot;                     /* its row in the tuner's audio array (refreshed when parameters are pushed) */
	DownConverter *mixer;
	LowPass *chanFilter;
	LowPass *chanFilter2;         /* a second LowPass in front of the demodulator, or NULL */
	Demodulator *demod;
	LowPass *audioFilter;
	bool dirty;                   /* parameters changed since the last submit */
	unsigned long long lateSeq;   /* the first block (counted from 1) submitted with the channel in `slot`: an
	                                 older ring entry's row `slot` is not this channel's (WEBRADIO_AUDIO_LATE) */
	/* for the SpectrumSinks on the chain's last channel filter: the channel-rate frames (at the demodulator's input) the
	 * tuner has been handed for this channel since it was enrolled, and how many of them the LAST submit brought */
	unsigned long long tapTotal, tapLast;
};

class TunerBatch {
public:
	/* enrol the Receiver chain that starts at `mixer` if the graph has that shape;
	 * returns the channel or NULL (-> the blocks run stand-alone) */
	static Channel *enrol(DownConverter *mixer);
	static void withdraw(Channel *ch);
	static void unfuseChainOf(DspBlock *block);
	/* the source is going (sourcestage.cxx: releaseSource): its batch and the batch's channels with it */
	static void destroyFor(DspSource *src);

	/* called from DownConverter::process of an enrolled block */
	bool submitOnce(const vector<sample_t> &tunerBuffer, unsigned int nframes);
	/* called from the audio LowPass::process of an enrolled block */
	bool audio(const Channel *ch, vector<sample_t> &out);
	/* a setter changed a parameter of this channel (any thread): re-stage it at the next
	 * block boundary */
	static void markDirty(Channel *ch);

	bool streamInfo(bool *live, unsigned long long *launches, unsigned long long *blocks);
	/* SpectrumSink::getSpectrum of a sink whose producer `filter` is the last channel filter of an enrolled chain: the dB row
	 * of the reference's most recent complete frame (spectrumframing.h), out of one wr_tuner_chan_spectra per (block,
	 * fft size, first frame) whose rows are downloaded once for every sink that asks.  `spec`: the sink's own wr_spectrum
	 * (its tables).  TAP_NONE: `filter` is in no batch -- the sink is fed samples and answers itself */
	enum Tap { TAP_NONE, TAP_SERVED, TAP_NOTHING_YET, TAP_FAILED };
	static Tap chanSpectrum(const DspBlock *filter, wr_spectrum *spec, unsigned int fftSize, unsigned int hop, float *magnitudes);
	static bool tapped(const DspBlock *filter) { return filter && filter->gpuChannel() != NULL; }
	unsigned long long chanSpectraCalls();
	/* Demodulator::inputLevel of an enrolled chain's demodulator: the mean and peak power (linear, full scale 1.0) of its
	 * input in the block submitted last -- with WEBRADIO_PIECES above 1 the block's last part -- out of ONE
	 * wr_tuner_chan_levels per block, whose arrays are kept until the next block for every Demodulator that asks.
	 * `muted` (optional): the audio frames of that submit the tuner's squelch muted.  TAP_NONE: `demod` is in no batch */
	static Tap chanLevel(const Demodulator *demod, float *mean, float *peak, unsigned int *muted = NULL);
	unsigned long long chanLevelCalls();
	bool streaming() const { return _streaming; }
	wr_dev *dev() const { return _dev; }
	DspSource *source() const { return _source; }
	size_t channels() const { return _channels.size(); }

private:
	TunerBatch(DspSource *source, wr_dev *dev);
	~TunerBatch();
	bool pushParams(Channel *ch);
	unsigned int piecesFor(unsigned int nframes);
	bool sparseWindows(unsigned int *period, unsigned int *length);
	enum Sent { SENT, FAILED, NOT_IN_PARTS };
	Sent submitParts(unsigned int parts, unsigned int nframes, const float *onDevice, const vector<sample_t> &host);
	bool submitOnePiece(const vector<sample_t> &tunerBuffer, unsigned int nframes, bool pushed);
	bool afterSubmit(bool pushed, unsigned int nframes);
	bool holdRingSlot();
	bool collectParts(unsigned int parts);
	void drainRing();
	void countTapFrames(unsigned int nframes, unsigned int parts);
	bool sinkQualifies(const SpectrumSink *sink, const LowPass *f1, const LowPass *f1b) const;
	static const Channel *tapChannel(const DspBlock *block, bool (*owns)(const Channel *, const DspBlock *),
	                                 std::unique_lock<std::mutex> &lock, Tap *answer);
	size_t rowsInUse() const;

	DspSource *_source;
	wr_dev *_dev;
	wr_tuner *_tuner;
	unsigned int _rate;
	size_t _maxFrames;
	unsigned long _submittedEpoch;
	bool _submitOk;
	std::vector<Channel *> _channels;
	std::vector<float> _audio;        /* [slot][frames] of the last submit (fallback without the ring) */
	const float *_audioPtr;           /* where audio() reads: a pinned ring slot, or _audio */
	bool _ringHeld;                   /* a slot of the tuner's pinned audio ring is acquired */
	size_t _audioStride, _audioFrames;
	unsigned int _audioSlots;
	bool _late;                       /* WEBRADIO_AUDIO_LATE: hand out the PREVIOUS block's audio (see submitOnce) */
	unsigned int _lateDepth;          /* 1: the previous block's audio; 2: the one before (no flush: one launch per block) */
	bool _lateQueued;                 /* a block has been submitted whose audio has not been handed out yet */
	bool _silence;                    /* late mode, first block: nothing to hand out yet */
	unsigned long long _lateSeq;      /* blocks submitted so far */
	unsigned int _pieces;             /* WEBRADIO_PIECES: parts an on-time block is put through in (see submitOnce) */
	bool _delivered;                  /* this block's audio already lies in the audio filters' output vectors */
	std::mutex _lock;
	unsigned long long _partSeq0;     /* the number the tuner gave the first part of the block collectParts is about to collect
	                                     (wr_tuner_submit_count before the parts went out: the library's own count) */
	bool _streaming;                  /* the source produces its blocks in device memory (DeviceBlock): wr_tuner_set_streaming */
	/* channel spectra of the block submitted last (_lateSeq), one entry per (fft size, first frame) asked about */
	struct TapRows {
		unsigned int n;
		unsigned long long first;
		unsigned int slots;
		std::vector<float> db;        /* [slots][n] */
	};
	std::vector<TapRows> _tapRows;
	unsigned long long _tapSeq;       /* the block (_lateSeq) _tapRows belongs to */
	unsigned long long _tapCalls;     /* wr_tuner_chan_spectra calls made */
	DevBuf _tapDev;
	/* signal levels of the block submitted last, by slot */
	std::vector<float> _lvMean, _lvPeak;
	std::vector<unsigned int> _lvMuted;
	unsigned int _lvSlots;
	unsigned long long _lvSeq;        /* the block (_lateSeq) they belong to; 0: none */
	unsigned long long _lvCalls;      /* wr_tuner_chan_levels calls made */
	/* WEBRADIO_TIMES=1 (measurement only): microseconds summed over `_timedBlocks` on-time blocks that went through in parts,
	 * by where they went (the destructor's line names the fields); `_submitStart`: when this block's submit began,
	 * `_lastCollected`: when the last block's parts had been collected */
	double _timeSums[7], _submitStart, _lastCollected;
	unsigned long _timedBlocks;
};

} // namespace wrhost

#endif /* WRHOST_GPUBATCH_H_ */
