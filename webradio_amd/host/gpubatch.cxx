/*
 * gpubatch.cxx -- see gpubatch.h.  Everything numerical happens behind the C ABI; this
 * file only decides WHAT is submitted WHEN, so that DspBlock::run()'s depth-first walk
 * (dspblock.cxx:207-209 upstream) ends up as one launch sequence per tuner block.
 */
#include "gpubatch.h"

#include <stdint.h>

#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <stdio.h>

#include "blockparts.h"
#include "debug.h"
#include "demodulator.h"
#include "downconverter.h"
#include "filetuner.h"
#include "lowpass.h"
#include "spectrumframing.h"
#include "spectrumsink.h"

namespace wrhost {

/* the tuner batch of `block`'s root source, or NULL */
static TunerBatch *batchOf(const DspBlock *block)
{
	DspSource *src = rootSource(block);
	return src ? src->batch() : NULL;
}

void submitBatchFirst(const DspBlock *consumer, const vector<sample_t> &host)
{
	TunerBatch *batch = batchOf(consumer);
	if (!batch || host.empty() || host.data() != batch->source()->currentBlock().data())
		return;
	if (batch->channels())
		(void)batch->submitOnce(host, (unsigned int)(host.size() / 2));      /* (the receivers see its verdict when they ask) */
}

bool streamInfo(const DspBlock *block, bool *live, unsigned long long *launches, unsigned long long *blocks)
{
	TunerBatch *batch = batchOf(block);
	return batch && batch->streamInfo(live, launches, blocks);
}

unsigned long long chanSpectraCalls(const DspBlock *block)
{
	TunerBatch *batch = batchOf(block);
	return batch ? batch->chanSpectraCalls() : 0;
}

unsigned long long chanLevelCalls(const DspBlock *block)
{
	TunerBatch *batch = batchOf(block);
	return batch ? batch->chanLevelCalls() : 0;
}

/* ------------------------------------------------------------------ TunerBatch -- */

/* WEBRADIO_TIMES=1 (measurement only): where the wall time of an on-time block goes inside the batch -- averaged and printed
 * when the batch goes (profiles/r05_host_times.txt) */
static const bool g_times = getenv("WEBRADIO_TIMES") && atoi(getenv("WEBRADIO_TIMES")) != 0;
static inline double nowUs()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

TunerBatch::TunerBatch(DspSource *source, wr_dev *dev)
	: _source(source), _dev(dev), _tuner(NULL), _rate(0), _maxFrames(0), _submittedEpoch(0),
	  _submitOk(false), _audioPtr(NULL), _ringHeld(false), _audioStride(0), _audioFrames(0), _audioSlots(0),
	  _late(envUnsigned("WEBRADIO_AUDIO_LATE", 0) != 0), _lateDepth(envUnsigned("WEBRADIO_AUDIO_LATE", 0) >= 2 ? 2u : 1u),
	  _lateQueued(false), _silence(false), _lateSeq(0), _pieces(envUnsigned("WEBRADIO_PIECES", 2)), _delivered(false), _partSeq0(0),
	  _streaming(false), _tapSeq(0), _tapCalls(0), _lvSlots(0), _lvSeq(0), _lvCalls(0), _timeSums(), _submitStart(0.0),
	  _lastCollected(0.0), _timedBlocks(0)
{
	if (_pieces < 1 || _late)
		_pieces = 1;
	if (_pieces > 8)
		_pieces = 8;
}

TunerBatch::~TunerBatch()
{
	const double *s = _timeSums;
	const unsigned long n = _timedBlocks;
	if (g_times && n)
		fprintf(stderr, "WEBRADIO_TIMES, us per block over %lu blocks: walk+source %.1f | stage enqueued %.1f | submits+flush %.1f (from the submit's start) | "
		        "wait part 0 %.1f copy %.1f | wait part 1 %.1f copy %.1f\n", n, s[0] / n, s[1] / n, s[2] / n,
		        s[3] / n, s[4] / n, s[5] / n, s[6] / n);
	if (_tuner)
		wr_tuner_destroy(_tuner);
}

void TunerBatch::destroyFor(DspSource *src)
{
	TunerBatch *b = src->batch();
	if (!b)
		return;
	src->setBatch(NULL);
	for (size_t n = 0; n < b->_channels.size(); n++)
		delete b->_channels[n];          /* their blocks are gone or stopping */
	b->_channels.clear();
	delete b;
}

/* The shape radio.cxx:68-76 builds, with nothing else attached along the way.  Only
 * then is it safe to skip the intermediate buffers. */

Channel *TunerBatch::enrol(DownConverter *mixer)
{
	DspBlock::gpuUnfuse = TunerBatch::unfuseChainOf;
	if (envUnsigned("WEBRADIO_NO_FUSION", 0))
		return NULL;
	DspSource *src = dynamic_cast<DspSource *>(mixer->_producer);
	if (!src || mixer->_consumers.size() != 1)
		return NULL;
	LowPass *f1 = dynamic_cast<LowPass *>(mixer->_consumers[0]);
	if (!f1 || f1->_consumers.empty())
		return NULL;
	/* optionally a second LowPass before the demodulator: how the reference's own means cut a narrow
	 * channel out of a fast stream (one 64-tap stage gives bin 0 below fs/128, lowpass.cxx:167) */
	LowPass *f1b = f1->_consumers.size() == 1 ? dynamic_cast<LowPass *>(f1->_consumers[0]) : NULL;
	/* the LAST channel stage feeds the demodulator and, beside it, any number of SpectrumSinks (a panadapter per listener:
	 * the channel spectrum).  Those get no samples: they are served out of the channel IQ the tuner keeps (chanSpectrum) */
	const LowPass *last = f1b ? f1b : f1;
	Demodulator *dm = NULL;
	std::vector<const SpectrumSink *> taps;
	for (size_t n = 0; n < last->_consumers.size(); n++) {
		DspBlock *c = last->_consumers[n];
		if (Demodulator *d = dynamic_cast<Demodulator *>(c)) {
			if (dm)
				return NULL;
			dm = d;
		} else if (const SpectrumSink *sink = dynamic_cast<const SpectrumSink *>(c)) {
			taps.push_back(sink);
		} else {
			return NULL;
		}
	}
	if (!dm || dm->_consumers.size() != 1)
		return NULL;
	LowPass *f2 = dynamic_cast<LowPass *>(dm->_consumers[0]);
	if (!f2)
		return NULL;
	if (f1->_channel || dm->_channel || f2->_channel || (f1b && f1b->_channel))
		return NULL;
	if (f1->firLength() > WR_FIR_FUSED_MAX || f2->firLength() > WR_FIR_FUSED_MAX ||
	    (f1b && f1b->firLength() > WR_FIR_FUSED_MAX))
		return NULL;                         /* the tuner takes the reference's 64 taps (shorter filters ride as 64 taps
		                                        with the oldest ones zero) and 128 or 256 for any of the three filters
		                                        (r05: the audio filter and the second channel stage too) */

	TunerBatch *batch = src->batch();
	if (!batch) {
		wr_dev *dev = deviceFor(mixer);      /* the source's GPU (tuners shard one per GPU) */
		if (!dev)
			return NULL;
		batch = new TunerBatch(src, dev);
		src->setBatch(batch);
	}

	for (size_t n = 0; n < taps.size(); n++)
		if (!batch->sinkQualifies(taps[n], f1, f1b))
			return NULL;                         /* block by block, the sink fed samples: the reference's dataflow */

	std::lock_guard<std::mutex> g(batch->_lock);
	{
		/* The wr_tuner outlives stop()/start() of the source (its channels park their state in
		 * their blocks meanwhile).  What a stopped source may have changed -- setSampleRate,
		 * setBlockSize (dspblock.h:60-66; refused while running) -- is baked into the tuner: the
		 * NCO step of every channel follows from the input rate (downconverter.cxx:80) and the
		 * device buffers are sized for the block.  With no channel enrolled nothing is lost by
		 * building a new one. */
		size_t wantFrames = src->blockSize() / 2;
		if (wantFrames == 0)
			wantFrames = 1;
		if (batch->_tuner && batch->_channels.empty() &&
		    (batch->_rate != src->outputSampleRate() || batch->_maxFrames != wantFrames)) {
			wr_tuner_destroy(batch->_tuner);
			batch->_tuner = NULL;
			batch->_ringHeld = false;
			batch->_audioSlots = 0;
			batch->_audioPtr = NULL;
			batch->_submitOk = false;
		}
	}
	if (!batch->_tuner) {
		batch->_rate = src->outputSampleRate();
		batch->_maxFrames = src->blockSize() / 2;
		if (batch->_maxFrames == 0)
			batch->_maxFrames = 1;
		unsigned int maxch = envUnsigned("WEBRADIO_MAX_CHANNELS", 1024);
		int nco = WR_NCO_ROTATE;
		const char *want = getenv("WEBRADIO_NCO");
		if (envUnsigned("WEBRADIO_NCO_EXACT", 0) || (want && !strcmp(want, "exact")))
			nco = WR_NCO_EXACT;
		else if (want && !strcmp(want, "split"))
			nco = WR_NCO_SPLIT;
		if (wr_tuner_create(&batch->_tuner, batch->_dev, batch->_rate, maxch, batch->_maxFrames, nco) != WR_OK) {
			LOG_ERROR("wr_tuner_create: %s\n", wr_last_error());
			batch->_tuner = NULL;
			return NULL;
		}
		wr_tuner_audio_ring(batch->_tuner, batch->_late ? 2 + batch->_lateDepth : 1 + (batch->_pieces > 1 ? batch->_pieces : 1));
		/* r06: a source that produces its blocks in device memory (DeviceBlock) is STREAMED: its blocks ring the doorbell of
		 * one persistent launch (k_tuner_stream, what bench.py's headline times) instead of launching a kernel each; a block's
		 * audio is in the pinned ring when WrStreamCtl::done says so, no flush.  Blocks that come out of HOST memory are
		 * staged by work on the device's own stream, which an open launch would hold up: they go the ordinary way.
		 * WEBRADIO_STREAM=0 turns it off. */
		batch->_streaming = dynamic_cast<DeviceBlock *>(src) != NULL && envUnsigned("WEBRADIO_STREAM", 1) != 0;
		if (batch->_streaming && wr_tuner_set_streaming(batch->_tuner, 1) != WR_OK)
			batch->_streaming = false;
		batch->_lateQueued = false;
		batch->_lateSeq = 0;
		batch->_tapRows.clear();
		batch->_tapSeq = 0;
		batch->_lvSeq = 0;
	}
	int id = -1;
	if (wr_chan_add(batch->_tuner, &id) != WR_OK) {
		LOG_ERROR("wr_chan_add: %s\n", wr_last_error());
		return NULL;
	}
	Channel *ch = new Channel();
	ch->batch = batch;
	ch->id = id;
	ch->slot = -1;
	ch->lateSeq = ~0ull;
	ch->tapTotal = ch->tapLast = 0;
	ch->mixer = mixer;
	ch->chanFilter = f1;
	ch->chanFilter2 = f1b;
	ch->demod = dm;
	ch->audioFilter = f2;
	ch->dirty = true;
	batch->_channels.push_back(ch);
	/* NCO phase and Demodulator prev_i/q outlive stop()/start() upstream (Q5) */
	wr_chan_set_state(batch->_tuner, id, mixer->_phase, dm->_prev);
	mixer->_channel = f1->_channel = dm->_channel = f2->_channel = ch;
	f1->_stage = 0;
	f2->_stage = 1;
	if (f1b) {
		f1b->_channel = ch;
		f1b->_stage = 2;
		f1b->elideOutput(true);
	}
	/* nobody reads these three on the host any more */
	mixer->elideOutput(true);
	f1->elideOutput(true);
	dm->elideOutput(true);
	return ch;
}

/* the decimation a LowPass that has not been started yet will have off `rate` (LowPass::init, DspBlock::start) */
static unsigned int decimationOff(unsigned int rate, unsigned int reqOutputRate, unsigned int reqDecimation, unsigned int *outRate)
{
	const unsigned int out = reqOutputRate ? reqOutputRate : (reqDecimation ? rate / reqDecimation : 0);
	*outRate = out;
	return out && out <= rate ? rate / out : 0;
}

/* May a SpectrumSink on the chain's last channel filter stay there while the chain is fused?  It is served the reference's
 * most recent complete frame out of the LAST submit's channel IQ: at most 8192 points (wr_tuner_chan_spectra), and the
 * smallest submit the batch makes for a source block -- the block, or one of WEBRADIO_PIECES parts of it -- holds
 * fftSize + hop channel-rate frames, so that the frame always lies inside it (spectrumframing.h). */
bool TunerBatch::sinkQualifies(const SpectrumSink *sink, const LowPass *f1, const LowPass *f1b) const
{
	const unsigned int n = sink->fftSize(), hop = sink->hop() ? sink->hop() : n;
	if (n < 8 || n > 8192 || hop > n)
		return false;
	unsigned int rate1 = 0, rate2 = 0;
	unsigned long d = decimationOff(_source->outputSampleRate(), f1->_reqOutputRate, f1->_reqDecimation, &rate1);
	if (f1b)
		d *= decimationOff(rate1, f1b->_reqOutputRate, f1b->_reqDecimation, &rate2);
	if (!d)
		return false;
	const unsigned long smallest = (_source->blockSize() / 2) / _pieces / d;
	return smallest >= (unsigned long)n + hop;
}

/* the block just submitted, in `parts` equal parts, as the channels' SpectrumSinks count it */
void TunerBatch::countTapFrames(unsigned int nframes, unsigned int parts)
{
	for (size_t n = 0; n < _channels.size(); n++) {
		Channel *c = _channels[n];
		if (c->slot < 0 || !c->chanFilter->isRunning() || (c->chanFilter2 && !c->chanFilter2->isRunning()))
			continue;
		const unsigned long d = (unsigned long)c->chanFilter->decimation() * (c->chanFilter2 ? c->chanFilter2->decimation() : 1u);
		c->tapLast = d ? (nframes / parts) / d : 0;          /* dspblock.cxx:177-178, stage after stage */
		c->tapTotal += c->tapLast * parts;
	}
}

unsigned long long TunerBatch::chanSpectraCalls()
{
	std::lock_guard<std::mutex> g(_lock);
	return _tapCalls;
}

/* What both taps begin with: the batch below whose source `block` runs is locked with `lock`, and the channel that `owns`
 * says `block` belongs to is looked up in the batch's own list under that lock (withdraw() may be taking the chain out on
 * another thread).  Returns the channel, seated in a slot of the batch's tuner (Channel::batch) -- or NULL and the tap's
 * `*answer`: TAP_NONE or TAP_NOTHING_YET. */
const Channel *TunerBatch::tapChannel(const DspBlock *block, bool (*owns)(const Channel *, const DspBlock *),
                                      std::unique_lock<std::mutex> &lock, Tap *answer)
{
	TunerBatch *b = batchOf(block);
	*answer = TAP_NONE;
	if (!b)
		return NULL;
	lock = std::unique_lock<std::mutex>(b->_lock);
	const Channel *ch = NULL;
	for (size_t n = 0; n < b->_channels.size() && !ch; n++)
		if (owns(b->_channels[n], block))
			ch = b->_channels[n];
	if (!ch || !b->_tuner)
		return NULL;
	*answer = TAP_NOTHING_YET;
	return ch->slot < 0 ? NULL : ch;
}

/* rows of room for every slot in use: the lane groups up to the highest one */
size_t TunerBatch::rowsInUse() const
{
	int top = 0;
	for (size_t n = 0; n < _channels.size(); n++)
		if (_channels[n]->slot > top)
			top = _channels[n]->slot;
	return ((size_t)top / 64 + 1) * 64;
}

TunerBatch::Tap TunerBatch::chanSpectrum(const DspBlock *filter, wr_spectrum *spec, unsigned int fftSize, unsigned int hop,
                                         float *magnitudes)
{
	std::unique_lock<std::mutex> g;
	Tap answer;
	const Channel *ch = tapChannel(filter, [](const Channel *c, const DspBlock *f) {
		return (c->chanFilter2 ? c->chanFilter2 : c->chanFilter) == f; }, g, &answer);
	if (!ch)
		return answer;
	TunerBatch *b = ch->batch;
	if (!ch->tapLast)
		return TAP_NOTHING_YET;
	unsigned long long first = 0;
	switch (spectrumFrameStart(ch->tapTotal, fftSize, hop, ch->tapLast, &first)) {
	case SPECTRUM_FRAME_NONE:
		return TAP_NOTHING_YET;
	case SPECTRUM_FRAME_AT:
		break;
	default:
		/* (a block shorter than the source's block size: the frame began in the block before, which is gone) */
		LOG_ERROR("SpectrumSink: the last block's %llu channel frames do not hold the most recent frame of %u\n",
		          ch->tapLast, fftSize);
		return TAP_FAILED;
	}
	if (b->_tapSeq != b->_lateSeq) {
		b->_tapRows.clear();
		b->_tapSeq = b->_lateSeq;
	}
	const TapRows *rows = NULL;
	for (size_t n = 0; n < b->_tapRows.size() && !rows; n++)
		if (b->_tapRows[n].n == fftSize && b->_tapRows[n].first == first)
			rows = &b->_tapRows[n];
	if (!rows) {
		const size_t room = b->rowsInUse();
		TapRows fresh;
		fresh.n = fftSize;
		fresh.first = first;
		fresh.slots = 0;
		++b->_tapCalls;
		if (!b->_tapDev.reserve(b->_dev, room * fftSize * sizeof(float)) ||
		    wr_tuner_chan_spectra(b->_tuner, spec, (size_t)first, (float *)b->_tapDev.ptr, &fresh.slots) != WR_OK ||
		    fresh.slots > room) {
			LOG_ERROR("SpectrumSink: wr_tuner_chan_spectra: %s\n", wr_last_error());
			return TAP_FAILED;
		}
		fresh.db.resize((size_t)fresh.slots * fftSize);
		if (wr_dev_download(b->_dev, fresh.db.data(), b->_tapDev.ptr, fresh.db.size() * sizeof(float)) != WR_OK) {
			LOG_ERROR("SpectrumSink: %s\n", wr_last_error());
			return TAP_FAILED;
		}
		b->_tapRows.push_back(fresh);
		rows = &b->_tapRows.back();
	}
	if ((unsigned int)ch->slot >= rows->slots)
		return TAP_FAILED;
	memcpy(magnitudes, rows->db.data() + (size_t)ch->slot * fftSize, fftSize * sizeof(float));
	return TAP_SERVED;
}

unsigned long long TunerBatch::chanLevelCalls()
{
	std::lock_guard<std::mutex> g(_lock);
	return _lvCalls;
}

TunerBatch::Tap TunerBatch::chanLevel(const Demodulator *demod, float *mean, float *peak, unsigned int *muted)
{
	std::unique_lock<std::mutex> g;
	Tap answer;
	const Channel *ch = tapChannel(demod, [](const Channel *c, const DspBlock *d) { return c->demod == d; }, g, &answer);
	if (!ch)
		return answer;
	TunerBatch *b = ch->batch;
	if (!b->_lateSeq)
		return TAP_NOTHING_YET;
	if (b->_lvSeq != b->_lateSeq) {
		const size_t room = b->rowsInUse();
		b->_lvMean.assign(room, 0.0f);
		b->_lvPeak.assign(room, 0.0f);
		b->_lvMuted.assign(room, 0u);
		b->_lvSlots = 0;
		b->_lvSeq = 0;
		++b->_lvCalls;
		size_t frames = 0;
		if (wr_tuner_chan_levels(b->_tuner, b->_lvMean.data(), b->_lvPeak.data(), b->_lvMuted.data(), &frames, NULL,
		                         &b->_lvSlots) != WR_OK || b->_lvSlots > room) {
			LOG_ERROR("Demodulator: wr_tuner_chan_levels: %s\n", wr_last_error());
			return TAP_FAILED;
		}
		if (!frames)
			return TAP_NOTHING_YET;
		b->_lvSeq = b->_lateSeq;
	}
	if ((unsigned int)ch->slot >= b->_lvSlots)
		return TAP_FAILED;
	*mean = b->_lvMean[ch->slot];
	*peak = b->_lvPeak[ch->slot];
	if (muted)
		*muted = b->_lvMuted[ch->slot];
	return TAP_SERVED;
}

/* DspBlock::connect on a block whose output the fusion had elided */
void TunerBatch::unfuseChainOf(DspBlock *block)
{
	withdraw(block->gpuChannel());
}

void TunerBatch::withdraw(Channel *ch)
{
	if (!ch)
		return;
	TunerBatch *batch = ch->batch;
	if (batch && batch->_tuner) {
		std::lock_guard<std::mutex> g(batch->_lock);
		wr_chan_get_state(batch->_tuner, ch->id, &ch->mixer->_phase, ch->demod->_prev);
		wr_chan_remove(batch->_tuner, ch->id);
		for (size_t n = 0; n < batch->_channels.size(); n++)
			if (batch->_channels[n] == ch) {
				batch->_channels.erase(batch->_channels.begin() + n);
				break;
			}
	}
	ch->mixer->_channel = NULL;
	if (ch->chanFilter2) {
		ch->chanFilter2->_channel = NULL;
		ch->chanFilter2->elideOutput(false);
	}
	ch->chanFilter->_channel = NULL;
	ch->demod->_channel = NULL;
	ch->audioFilter->_channel = NULL;
	ch->mixer->elideOutput(false);
	ch->chanFilter->elideOutput(false);
	ch->demod->elideOutput(false);
	delete ch;
}

void TunerBatch::markDirty(Channel *ch)
{
	if (!ch)
		return;
	std::lock_guard<std::mutex> g(ch->batch->_lock);
	ch->dirty = true;
}

/* stage the block-level parameters of one channel (setters may have run on other
 * threads since the last block; they take effect here, at a block boundary) */
bool TunerBatch::pushParams(Channel *ch)
{
	LowPass *f1 = ch->chanFilter, *f2 = ch->audioFilter;
	if (!f1->isRunning() || !f2->isRunning() || !ch->demod->isRunning() ||
	    (ch->chanFilter2 && !ch->chanFilter2->isRunning()))
		return true;                    /* the chain is still starting: next block */
	if (wr_chan_set_if(_tuner, ch->id, ch->mixer->_ifHz) != WR_OK)
		return false;
	LowPass *fs[3] = {f1, ch->chanFilter2, f2};
	const int stages[3] = {WR_FILTER_CHANNEL, WR_FILTER_CHANNEL2, WR_FILTER_AUDIO};
	for (int n = 0; n < 3; n++) {
		if (!fs[n])
			continue;
		vector<float> taps;
		{
			std::lock_guard<std::mutex> g(fs[n]->_coeffLock);          /* see LowPass::recalculate */
			taps = fs[n]->_coeff;
		}
		if (!taps.empty() && taps.size() <= (size_t)WR_FIR_FUSED_MAX &&
		    wr_chan_set_taps_n(_tuner, ch->id, stages[n], taps.data(), (unsigned int)taps.size(),
		                       fs[n]->decimation()) != WR_OK)
			return false;
	}
	if (wr_chan_set_mode(_tuner, ch->id, (int)ch->demod->_mode) != WR_OK)
		return false;
	ch->dirty = false;
	return true;
}

bool TunerBatch::submitOnce(const vector<sample_t> &tunerBuffer, unsigned int nframes)
{
	std::lock_guard<std::mutex> g(_lock);
	if (_submittedEpoch == _source->epoch())
		return _submitOk;
	_submittedEpoch = _source->epoch();
	_submitOk = false;
	/* 1. what the setters changed since the last block */
	bool pushed = false;
	for (size_t n = 0; n < _channels.size(); n++)
		if (_channels[n]->dirty || _channels[n]->slot < 0) {
			pushed = true;
			if (_channels[n]->dirty && !pushParams(_channels[n])) {
				LOG_ERROR("channel parameters rejected: %s\n", wr_last_error());
				return false;
			}
		}
	if (nframes > _maxFrames) {
		LOG_ERROR("block of %u frames exceeds the %zu the tuner batch was sized for\n", nframes, _maxFrames);
		return false;
	}
	if (_ringHeld) {
		wr_tuner_audio_ring_release(_tuner);      /* last block's audio has been handed out */
		_ringHeld = false;
		_audioSlots = 0;
	}
	_delivered = false;
	/* 2. how the block goes.  On time (the default: a block's audio is handed on within the run() that brought the block) it
	 * goes through in P equal parts: part p + 1 crosses PCIe while part p's kernels run, part p's audio comes back -- and is put
	 * where the audio filters' consumers will read it -- while part p + 1 computes.  What run() then waits for after the link
	 * has delivered the block is one part's kernels and transfer, not the block's (r03: transfer, kernels, audio copy
	 * and hand-out in series, 0.43 ms a C2 block of bytes; the bits do not depend on how a stream is cut into blocks:
	 * tests/test_gpu_tuner.py::test_block_split_invariance). */
	/* (r04) Where every receiver decimates alike and by at least twice its channel filter's length, only the frames under
	 * the taps are brought over (stagedSparse): a sixth of the block at BASELINE config 2 -- and no transfer to wait for. */
	const unsigned int parts = pushed ? 1u : piecesFor(nframes);
	Sent sent = NOT_IN_PARTS;
	unsigned int sp = 0, sl = 0;
	_submitStart = g_times ? nowUs() : 0.0;
	if (g_times && _lastCollected > 0.0)
		_timeSums[0] += _submitStart - _lastCollected;      /* from the end of the last collectParts to this submit: the walk + the source */
	if (!pushed && sparseWindows(&sp, &sl)) {
		wr_dev *sdev = NULL;
		const float *staged = stagedSparse(_channels[0]->mixer, tunerBuffer, &sdev, sp, sl, sl - 1u);
		if (g_times)
			_timeSums[1] += nowUs() - _submitStart;             /* staging enqueued */
		/* on time, the staged block goes through in P parts all the same: a part's audio is put where the audio
		 * filters' consumers will read it while the parts behind it compute (collectParts) */
		if (staged && sdev == _dev)
			sent = submitParts(parts, nframes, staged, tunerBuffer);
	}
	/* 3. submit and collect: the sparse-staged block above, else in parts staged one by one, else in one piece */
	if (sent == NOT_IN_PARTS && parts > 1)
		sent = submitParts(parts, nframes, NULL, tunerBuffer);
	return sent == NOT_IN_PARTS ? submitOnePiece(tunerBuffer, nframes, pushed) : sent == SENT;
}

/* The block in `parts` equal parts, one submit each, and their audio collected.  `onDevice`: the block lies there already
 * (sparse-staged, or a DeviceBlock source's), part p a stride behind part p - 1; NULL: it is in host memory and part p is
 * staged just before it is submitted (stagePiece).  NOT_IN_PARTS: the block cannot be staged in parts and nothing has been
 * submitted -- the caller takes the one-piece path. */
TunerBatch::Sent TunerBatch::submitParts(unsigned int parts, unsigned int nframes, const float *onDevice, const vector<sample_t> &host)
{
	const unsigned int each = nframes / parts;
	wr_tuner_submit_count(_tuner, &_partSeq0);      /* part p's ring entry will be numbered _partSeq0 + p: the library's count */
	for (unsigned int p = 0; p < parts; p++) {
		const float *part = onDevice ? onDevice + (size_t)2 * each * p : stagePiece(_source, _dev, host, parts, p);
		if (!part)
			return p ? FAILED : NOT_IN_PARTS;
		if (wr_tuner_submit(_tuner, part, each, WR_DEVICE) != WR_OK) {
			if (onDevice)
				LOG_ERROR("wr_tuner_submit: %s\n", wr_last_error());
			else
				LOG_ERROR("wr_tuner_submit (part %u of %u): %s\n", p, parts, wr_last_error());
			if (p)
				drainRing();                /* the parts that did go out must not be taken for the next block's */
			return FAILED;
		}
	}
	if (parts == 1)
		return afterSubmit(false, nframes) ? SENT : FAILED;
	countTapFrames(nframes, parts);
	++_lateSeq;
	/* the last part's demodulator + audio filter: nothing rides behind it.  Only a streaming launch's post stage starts by
	 * itself, and only a block that lies on the device is streamed: one out of host memory is always flushed */
	if (!(onDevice && _streaming))
		wr_tuner_flush(_tuner);
	traceAdd(_source, 'S');
	if (g_times && onDevice)
		_timeSums[2] += nowUs() - _submitStart;     /* ... parts submitted and flushed */
	return collectParts(parts) ? SENT : FAILED;
}

/* the block in one submit, by the cheapest way to get it to the GPU: (1) a device copy some other consumer of the
 * source already made this block, (2) the source's raw bytes (2 per frame, converted in
 * the kernel's load stage), (3) stage the float block once for everybody */
bool TunerBatch::submitOnePiece(const vector<sample_t> &tunerBuffer, unsigned int nframes, bool pushed)
{
	wr_dev *sdev = NULL;
	int rc;
	const float *staged = _channels.empty() ? NULL : stagedBlockIfPresent(_channels[0]->mixer, tunerBuffer, &sdev);
	const uint8_t *bytes = staged ? NULL : rawBytesOf(_source, (size_t)2 * nframes);
	if (staged && sdev == _dev) {
		rc = wr_tuner_submit(_tuner, staged, nframes, WR_DEVICE);
	} else if (bytes && envUnsigned("WEBRADIO_NO_U8_STAGING", 0)) {
		/* (the other way round than in sourcestage.cxx, on purpose: with the switch UNSET the bytes are staged and converted
		 * for every consumer, (3); with it set nothing stages them, and the tuner takes them from the host itself) */
		rc = wr_tuner_submit_u8(_tuner, bytes, nframes, WR_HOST);
	} else {
		staged = _channels.empty() ? NULL : stagedBlock(_channels[0]->mixer, tunerBuffer, &sdev);
		if (!(staged && sdev == _dev) && !_source->hostBlockValid()) {
			LOG_ERROR("the source left its block on the device and the device copy is not there\n");
			return false;
		}
		rc = (staged && sdev == _dev) ? wr_tuner_submit(_tuner, staged, nframes, WR_DEVICE)
		                              : wr_tuner_submit(_tuner, tunerBuffer.data(), nframes, WR_HOST);
	}
	if (rc != WR_OK) {
		LOG_ERROR("wr_tuner_submit: %s\n", wr_last_error());
		return false;
	}
	return afterSubmit(pushed, nframes);
}

bool TunerBatch::streamInfo(bool *live, unsigned long long *launches, unsigned long long *blocks)
{
	std::lock_guard<std::mutex> g(_lock);
	int l = 0;
	unsigned long long a = 0, b = 0;
	if (!_tuner || wr_tuner_stream_info(_tuner, &l, &a, &b) != WR_OK)
		return false;
	if (live)
		*live = l != 0;
	if (launches)
		*launches = a;
	if (blocks)
		*blocks = b;
	return true;
}

/* do all receivers read the source block through windows of one shape -- the same decimation, the same channel-filter
 * length -- and sparsely enough for sparse staging to pay (a window at most every second filter length)? */
bool TunerBatch::sparseWindows(unsigned int *period, unsigned int *length)
{
	if (_channels.empty())
		return false;
	unsigned int d = 0, l = 0;
	for (size_t n = 0; n < _channels.size(); n++) {
		const LowPass *f = _channels[n]->chanFilter;
		if (!f->isRunning() || _channels[n]->slot < 0)
			return false;
		const unsigned int dn = f->decimation(), ln = f->firLength();
		if (n == 0) {
			d = dn;
			l = ln;
		} else if (dn != d || ln != l) {
			return false;
		}
	}
	if (l < 2 || d < 2 * l)
		return false;
	*period = d;
	*length = l;
	return true;
}

/* the block has been submitted (enqueued): bookkeeping, and this run()'s audio */
bool TunerBatch::afterSubmit(bool pushed, unsigned int nframes)
{
	++_lateSeq;                            /* blocks submitted so far */
	if (pushed)                            /* a filter change may have moved a channel to another rate group */
		for (size_t n = 0; n < _channels.size(); n++) {
			const int before = _channels[n]->slot;
			if (wr_chan_slot(_tuner, _channels[n]->id, &_channels[n]->slot) != WR_OK)
				_channels[n]->slot = -1;
			if (_channels[n]->slot != before)
				_channels[n]->lateSeq = _lateSeq;          /* this block is the first in that slot: the ring entry
				                                              of the block before it is not this channel's */
		}
	countTapFrames(nframes, 1);
	/* the graph hands this block's audio on within this very run(): no waiting for the next launch.
	 * (WEBRADIO_AUDIO_LATE=2 hands out the audio of the block before the previous one: the demodulator and
	 * audio filter of a block then ride in the NEXT block's launch, as in bench.py -- one launch per block.) */
	if (!(_late && _lateDepth >= 2) && !_streaming)
		wr_tuner_flush(_tuner);                /* (a flush would close a streaming launch, every block: its post stage needs none) */
	traceAdd(_source, 'S');
	{
		int ready = 0;
		if (traceOn() && (!_late || _lateSeq > _lateDepth) && wr_tuner_audio_ring_ready(_tuner, &ready) == WR_OK)
			traceAdd(_source, ready ? 'A' : 'W');
	}
	if (_late) {
		/* WEBRADIO_AUDIO_LATE=1 (2): the sinks get every block's audio ONE run() (TWO) later (a block's worth
		 * of latency, 40 ms at C2).  Nothing in run() then waits for the GPU: this block's copy,
		 * kernels and audio transfer are merely enqueued, what is handed out is the previous
		 * block's audio, which arrived in the pinned ring while the host was busy elsewhere -- and
		 * the front ends of a Radio (radio.cxx:56-59 pumps them one after the other) keep all their
		 * GPUs busy at once.  The first block's run() hands out silence, the last block's audio is
		 * dropped at stop(). */
		_silence = _lateSeq <= _lateDepth;          /* (blocks submitted so far, this one included) */
		_lateQueued = true;
		_audioSlots = 0;
		if (!_silence)
			(void)holdRingSlot();
			/* (not held: nothing queued -- receivers in several rate groups are not ringed (see the C ABI);
			 * audio() then fetches per channel, which is this block's audio, on time) */
		_submitOk = true;
		return true;
	}
	/* one transfer brings back the audio of every channel: through the tuner's pinned ring
	 * (queued behind the kernels by the submit itself), read in place until the next block */
	if (holdRingSlot()) {
		_submitOk = true;
		return true;
	}
	size_t stride = 0, frames = 0;
	unsigned int slots = 0;
	if (wr_tuner_fetch_audio_all(_tuner, NULL, 0, &stride, &frames, &slots) != WR_OK && frames * slots == 0) {
		/* several rate groups: fall back to per-channel fetches in audio() */
		_audioSlots = 0;
		_submitOk = true;
		return true;
	}
	_audio.resize((size_t)slots * frames + 1);
	if (frames != 0 && slots != 0 &&
	    wr_tuner_fetch_audio_all(_tuner, _audio.data(), _audio.size(), &stride, &frames, &slots) != WR_OK) {
		_audioSlots = 0;                /* per-channel fallback */
	} else {
		_audioPtr = _audio.data();
		_audioStride = stride;
		_audioFrames = frames;
		_audioSlots = slots;
	}
	_submitOk = true;
	return true;
}

/* take the oldest entry of the tuner's pinned audio ring (waiting for it to land) and remember where audio() reads it;
 * false: there is none */
bool TunerBatch::holdRingSlot()
{
	const float *p = NULL;
	size_t stride = 0, frames = 0;
	unsigned int slots = 0;
	unsigned long long seq = 0;
	if (wr_tuner_audio_ring_acquire(_tuner, &p, &stride, &frames, &slots, &seq) != WR_OK)
		return false;
	_ringHeld = true;
	_audioPtr = p;
	_audioStride = stride;
	_audioFrames = frames;
	_audioSlots = slots;
	return true;
}

/* in how many equal parts a block of `nframes` goes through (submitOnce): as many as WEBRADIO_PIECES allows (default 2: each further part costs a launch and a transfer of
 * its own, ~30 us, more than its overlap saves -- profiles/r04_host_pieces.txt;
 * 1 turns it off) such that every part is a whole number of audio frames of every receiver, all receivers decimate alike
 * (one rate group: the tuner's pinned audio ring then carries every part's audio) and a part stays large enough for the
 * link and the kernels to work at their pace (WEBRADIO_PIECE_MIN_FRAMES, default 500 000) */
unsigned int TunerBatch::piecesFor(unsigned int nframes)
{
	if (_pieces <= 1 || _late || _channels.empty() || !nframes)
		return 1;
	unsigned long q = 1;
	unsigned int d[3] = {0, 0, 0};
	for (size_t n = 0; n < _channels.size(); n++) {
		const Channel *c = _channels[n];
		if (c->slot < 0 || !c->chanFilter->isRunning() || !c->audioFilter->isRunning())
			return 1;
		const unsigned int e[3] = {c->chanFilter->decimation(), c->chanFilter2 ? c->chanFilter2->decimation() : 1u,
		                           c->audioFilter->decimation()};
		if (n == 0)
			memcpy(d, e, sizeof(d));
		else if (memcmp(d, e, sizeof(d)))
			return 1;
		q = lcmCapped(q, (unsigned long)e[0] * e[1] * e[2]);
		if (!q)
			return 1;
	}
	static const unsigned int minFrames = envUnsigned("WEBRADIO_PIECE_MIN_FRAMES", 500000);
	return partsOf(nframes, _pieces, q, minFrames);
}

/* the audio of the P parts just submitted, in order: each part's rows are copied out of the tuner's pinned ring as soon as
 * they are there -- straight into the audio filters' output vectors where those already have the block's size (the steady
 * state: LowPass::process then has nothing left to copy), else into _audio for audio() to slice -- while the parts behind
 * it are still being worked on.  r05: a ring entry that is not the part expected -- a leftover of a run() that failed half
 * way -- is an error, not somebody else's audio.  (Helper threads for the copies were tried and taken out again: 256 rows of
 * 4 KB per part are 30-40 us of one core, but what an on-time block waits for is the GPU -- WEBRADIO_TIMES=1 says where the
 * time goes: profiles/r05_host_times.txt.) */
bool TunerBatch::collectParts(unsigned int P)
{
	size_t off = 0, total = 0;
	bool direct = true;
	for (unsigned int p = 0; p < P; p++) {
		const float *ptr = NULL;
		size_t stride = 0, frames = 0;
		unsigned int slots = 0;
		unsigned long long seq = 0;
		const double ta = g_times ? nowUs() : 0.0;
		if (wr_tuner_audio_ring_acquire(_tuner, &ptr, &stride, &frames, &slots, &seq) != WR_OK) {
			LOG_ERROR("audio of part %u of %u: %s\n", p, P, wr_last_error());
			drainRing();
			return false;
		}
		const double tb = g_times ? nowUs() : 0.0;
		if (g_times)
			_timeSums[p ? 5 : 3] += tb - ta;           /* waiting for the part's audio */
		if (p == 0) {
			total = frames * P;
			for (size_t n = 0; n < _channels.size() && direct; n++)
				direct = _channels[n]->slot >= 0 && (unsigned int)_channels[n]->slot < slots &&
				         _channels[n]->audioFilter->DspBlock::_out.size() == total;
			if (!direct)
				_audio.resize((size_t)slots * total + 1);
			_audioSlots = slots;
		}
		/* the tuner numbers its submits from 0: part p of this block is submit _partSeq0 + p */
		if (frames * P != total || slots != _audioSlots || seq != _partSeq0 + p) {
			wr_tuner_audio_ring_release(_tuner);
			LOG_ERROR("part %u of %u came back as submit %llu with %zu frames (expected submit %llu, %zu frames): stale ring entries\n",
			          p, P, seq, frames, _partSeq0 + p, total / P);
			drainRing();
			return false;
		}
		if (direct) {
			for (size_t n = 0; n < _channels.size(); n++)
				memcpy(_channels[n]->audioFilter->DspBlock::_out.data() + off, ptr + (size_t)_channels[n]->slot * stride,
				       frames * sizeof(float));
		} else {
			for (unsigned int sl = 0; sl < slots; sl++)
				memcpy(_audio.data() + (size_t)sl * total + off, ptr + (size_t)sl * stride, frames * sizeof(float));
		}
		wr_tuner_audio_ring_release(_tuner);
		off += frames;
		if (g_times)
			_timeSums[p ? 6 : 4] += nowUs() - tb;      /* copying it out */
	}
	if (g_times) {
		_lastCollected = nowUs();
		++_timedBlocks;
	}
	_ringHeld = false;
	_audioFrames = total;
	if (direct) {
		_delivered = true;
	} else {
		_audioPtr = _audio.data();
		_audioStride = total;
	}
	_submitOk = true;
	return true;
}

/* whatever is queued in the tuner's audio ring goes: after an error half way through a block its entries would be taken
 * for the next block's parts */
void TunerBatch::drainRing()
{
	wr_tuner_flush(_tuner);
	for (;;) {
		unsigned int queued = 0;
		if (wr_tuner_audio_ring_stats(_tuner, &queued, NULL) != WR_OK || !queued)
			break;
		const float *ptr = NULL;
		size_t stride = 0, frames = 0;
		unsigned int slots = 0;
		if (wr_tuner_audio_ring_acquire(_tuner, &ptr, &stride, &frames, &slots, NULL) != WR_OK)
			break;
		wr_tuner_audio_ring_release(_tuner);
	}
	_ringHeld = false;
}

bool TunerBatch::audio(const Channel *ch, vector<sample_t> &out)
{
	/* under the batch lock: withdraw() / unfuseChainOf() may run on an HTTP thread (a consumer connected
	 * inside a fused chain) while the run thread hands audio out; uncontended it costs 256 x ~20 ns a block */
	std::lock_guard<std::mutex> g(_lock);
	if (!_submitOk)
		return false;
	if (out.empty())
		return true;
	if (_delivered && out.size() == _audioFrames && out.data() == ch->audioFilter->DspBlock::_out.data())
		return true;                            /* collectParts put it there while the block's last parts were computing */
	if (_late && _silence) {
		memset(out.data(), 0, out.size() * sizeof(float));
		return true;
	}
	const int slot = ch->slot;
	if (_audioSlots && slot >= 0 && (unsigned int)slot < _audioSlots && _audioFrames == out.size() &&
	    (!_late || ch->lateSeq + (_lateDepth - 1u) < _lateSeq)) {
		memcpy(out.data(), _audioPtr + (size_t)slot * _audioStride, out.size() * sizeof(float));
		return true;
	}
	if (_late && _audioSlots) {
		/* One block late, and the ring entry is not this channel's previous block: another block length
		 * (a ragged block, a changed audio rate), or a channel enrolled (or moved to this slot) with the
		 * block just submitted, whose slot held somebody else's audio a block ago.  Fetching now would hand
		 * out the CURRENT block -- and the next run() the same block again from the ring.  The sinks get a
		 * block of silence instead, exactly as at the start of the stream. */
		memset(out.data(), 0, out.size() * sizeof(float));
		return true;
	}
	size_t got = 0;
	if (wr_chan_fetch(_tuner, ch->id, WR_STAGE_AUDIO, out.data(), out.size(), &got) != WR_OK) {
		LOG_ERROR("wr_chan_fetch: %s\n", wr_last_error());
		return false;
	}
	return got == out.size();
}

} // namespace wrhost
