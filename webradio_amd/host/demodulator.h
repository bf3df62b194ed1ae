/*
 * demodulator.h -- IQ -> mono detector (AM / FM / USB / LSB).  Public surface of
 * webradio's src/dsp/demodulator.h:34-51, including the block type string "AMDemod".
 */
#ifndef DEMODULATOR_H_
#define DEMODULATOR_H_

#include <mutex>
#include <string>
#include <vector>

#include "dspblock.h"

using namespace std;

namespace wrhost { class TunerBatch; struct Channel; struct DevBuf; }

class Demodulator : public DspBlock
{
	friend class wrhost::TunerBatch;
public:
	Demodulator(const string &name = "<undefined>");
	virtual ~Demodulator();

	enum Mode {
		AM,
		FM,
		USB,
		LSB,
		MAX_MODE
	};

	const Mode mode() const { return _mode; }
	void setMode(const Mode mode);
	const string& modeString() const { return _modeNames[_mode]; }
	bool setModeString(const string &mode);

	/* extension (an S-meter beside the squelch_threshold and af_gain the reference's REST interface names,
	 * web/receiverhandler.cxx:112,118-119): the level of the demodulator's most recent input block, 10 * log10 of the mean
	 * and of the largest i*i + q*q in dBFS (computed on the host in double; a silent channel gives -inf, as the
	 * spectrum's dB rows do).  Any thread.  false: nothing to report yet.
	 *   Inside the tuner batch: the last submit's channel IQ -- with WEBRADIO_PIECES above 1 the block's LAST part --
	 * measured for every receiver of the tuner by one wr_tuner_chan_levels per block; before the first submit false; a
	 * call beside an open streaming launch closes it, as a channel-spectrum poll does.
	 *   Stand-alone: the first call answers false and asks for the measurement; from the next process() on every block
	 * is measured (wr_iq_levels) and the call answers with the latest.  A chain nobody asks costs nothing more. */
	bool inputLevel(float *mean_dbfs, float *peak_dbfs);

private:
	bool init();
	void deinit();
	bool process(const vector<sample_t> &inBuffer, vector<sample_t> &outBuffer);
	bool acceptsDeviceInput() const { return _channel == NULL; }   /* stand-alone: reads the producer's device output */
	wrhost::Channel *gpuChannel() const { return _channel; }

	Mode			_mode;
	vector<string>	_modeNames;
	float			_prev[2];		/* prev_i, prev_q: survive stop()/start() (quirk Q5) */
	wrhost::Channel*	_channel;
	wrhost::DevBuf*	_in;
	wrhost::DevBuf*	_out;
	std::mutex		_levelLock;		/* the three below: inputLevel() may come from an HTTP thread, like the setters */
	bool			_levelWanted, _levelHave;
	float			_level[2];		/* mean, peak: linear */
};

#endif /* DEMODULATOR_H_ */
