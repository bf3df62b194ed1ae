/*
 * audio_spectrum.cxx -- a receiver's AUDIO spectrum through the host runtime: FileTuner -> Receiver with a SpectrumSink
 * (one channel: the reference's FIXMEs at io/spectrumsink.cxx:62-64) and the retaining AudioStreamManager both behind the
 * audio filter.  TEST DRIVER (tests/test_gpu_host_audio_spectrum.py compiles and runs it).
 *
 *   audio_spectrum <recording.u8> <out prefix> <rate> <block_frames> <blocks> <if_hz> <fft_size> <iq_sink: 0|1>
 *
 * writes <out>.audio (the audio retained, floats), <out>.row (the audio sink's getSpectrum row), with iq_sink = 1 also
 * <out>.iqrow (the row of a second sink of the same size on the tuner itself: two channels), and prints
 * wr_block_kernel_calls(): 0 while the receiver stayed in the tuner batch.
 */
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "filetuner.h"
#include "radio.h"

static bool dump(const std::string &path, const float *v, size_t n)
{
	FILE *f = fopen(path.c_str(), "wb");
	if (!f)
		return false;
	const bool ok = fwrite(v, sizeof(float), n, f) == n;
	return fclose(f) == 0 && ok;
}

int main(int argc, char **argv)
{
	if (argc != 9) {
		fprintf(stderr, "usage: audio_spectrum recording out rate block_frames blocks if_hz fft_size iq_sink\n");
		return 2;
	}
	const std::string out = argv[2];
	const unsigned int rate = atoi(argv[3]), frames = atoi(argv[4]), blocks = atoi(argv[5]), fft = atoi(argv[7]);
	const bool iqSink = atoi(argv[8]) != 0;

	FrontEnd *fe = new FrontEnd(FileTuner::factory);
	Tuner *tuner = fe->tuner();
	tuner->setSubdevice(argv[1]);
	tuner->setSampleRate(rate);
	tuner->setChannels(2);
	tuner->setBlockSize(frames * 2);
	Receiver *rx = new Receiver();                 /* radio.cxx's defaults: 240 kHz channel, 48 kHz audio */
	rx->downconverter()->setIF(atoi(argv[6]));
	rx->demodulator()->setMode(Demodulator::FM);
	SpectrumSink *audioSink = new SpectrumSink("audio");
	audioSink->setFftSize(fft);
	rx->audioFilter()->connect(audioSink);
	SpectrumSink *tunerSink = NULL;
	if (iqSink) {
		tunerSink = new SpectrumSink("iq");
		tunerSink->setFftSize(fft);
		tuner->connect(tunerSink);
	}
	rx->setFrontEnd(fe);
	if (!tuner->start()) {
		fprintf(stderr, "start failed\n");
		return 1;
	}
	if (audioSink->inputChannels() != 1 || (tunerSink && tunerSink->inputChannels() != 2)) {
		fprintf(stderr, "unexpected channel counts\n");
		return 1;
	}
	for (unsigned int b = 0; b < blocks; b++)
		if (!tuner->run()) {
			fprintf(stderr, "run %u failed\n", b);
			return 1;
		}
	std::vector<float> row(fft, -1.0f), iqrow(fft, -1.0f);
	audioSink->getSpectrum(row.data());
	if (tunerSink)
		tunerSink->getSpectrum(iqrow.data());
	const std::vector<float> &audio = rx->stream()->samples();
	bool ok = dump(out + ".audio", audio.data(), audio.size()) && dump(out + ".row", row.data(), row.size());
	if (tunerSink)
		ok = ok && dump(out + ".iqrow", iqrow.data(), iqrow.size());
	printf("{\"block_kernel_calls\": %llu, \"audio_samples\": %lu}\n", wr_block_kernel_calls(),
	       rx->stream()->totalSamples());
	tuner->stop();
	delete rx;
	delete fe;
	delete audioSink;
	delete tunerSink;
	return ok ? 0 : 1;
}
