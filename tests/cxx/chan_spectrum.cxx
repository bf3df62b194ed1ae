/*
 * chan_spectrum.cxx -- every receiver's CHANNEL spectrum through the host runtime: FileTuner -> R Receivers, each with a
 * SpectrumSink on its channel filter (the signal the demodulator sees; a panadapter per listener).  TEST DRIVER
 * (tests/test_gpu_host_chan_spectrum.py compiles and runs it).
 *
 *   chan_spectrum <recording.u8> <out prefix> <rate> <block_frames> <blocks> <fft_size> <if_hz>...
 *
 * runs <blocks> blocks, reads every sink once, writes <out>.rows (one getSpectrum row per receiver, in the order of the
 * IFs; a row nobody filled stays at -1) and prints wr_block_kernel_calls() -- 0 while the receivers stayed in the tuner
 * batch -- and the wr_tuner_chan_spectra calls the batch made for those reads.
 */
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "filetuner.h"
#include "gpubatch.h"
#include "radio.h"

int main(int argc, char **argv)
{
	if (argc < 8) {
		fprintf(stderr, "usage: chan_spectrum recording out rate block_frames blocks fft_size if_hz...\n");
		return 2;
	}
	const std::string out = argv[2];
	const unsigned int rate = atoi(argv[3]), frames = atoi(argv[4]), blocks = atoi(argv[5]), fft = atoi(argv[6]);
	const size_t R = argc - 7;

	FrontEnd *fe = new FrontEnd(FileTuner::factory);
	Tuner *tuner = fe->tuner();
	tuner->setSubdevice(argv[1]);
	tuner->setSampleRate(rate);
	tuner->setChannels(2);
	tuner->setBlockSize(frames * 2);
	std::vector<Receiver *> rx(R);
	std::vector<SpectrumSink *> sink(R);
	for (size_t r = 0; r < R; r++) {
		rx[r] = new Receiver();                    /* radio.cxx's defaults: 240 kHz channel, 48 kHz audio */
		rx[r]->downconverter()->setIF(atoi(argv[7 + r]));
		rx[r]->demodulator()->setMode(Demodulator::FM);
		sink[r] = new SpectrumSink("channel");
		sink[r]->setFftSize(fft);
		rx[r]->channelFilter()->connect(sink[r]);
		rx[r]->setFrontEnd(fe);
	}
	if (!tuner->start()) {
		fprintf(stderr, "start failed\n");
		return 1;
	}
	for (unsigned int b = 0; b < blocks; b++)
		if (!tuner->run()) {
			fprintf(stderr, "run %u failed\n", b);
			return 1;
		}
	std::vector<float> rows(R * fft, -1.0f);
	for (size_t r = 0; r < R; r++)
		sink[r]->getSpectrum(rows.data() + r * fft);
	const unsigned long long spectraCalls = wrhost::chanSpectraCalls(rx[0]->downconverter());
	FILE *f = fopen((out + ".rows").c_str(), "wb");
	bool ok = f && fwrite(rows.data(), sizeof(float), rows.size(), f) == rows.size();
	ok = f && fclose(f) == 0 && ok;
	printf("{\"block_kernel_calls\": %llu, \"spectra_calls\": %llu, \"audio_samples\": %lu}\n", wr_block_kernel_calls(),
	       spectraCalls, rx[0]->stream()->totalSamples());
	tuner->stop();
	for (size_t r = 0; r < R; r++)
		delete rx[r];
	delete fe;
	for (size_t r = 0; r < R; r++)
		delete sink[r];
	return ok ? 0 : 1;
}
