/*
 * chan_level.cxx -- every receiver's signal level through the host runtime: FileTuner -> R Receivers, each asked for
 * demodulator()->inputLevel() after every block.  TEST DRIVER (tests/test_gpu_host_chan_level.py compiles and runs it).
 *
 *   chan_level <recording.u8> <rate> <block_frames> <blocks> <ask 0|1> <if_hz>...
 *
 * prints one JSON line: "answers" -- per block, per receiver (in the order of the IFs) [answered, the bits of mean_dbfs,
 * the bits of peak_dbfs] --, wr_block_kernel_calls() (0 while the receivers stayed in the tuner batch) and the
 * wr_tuner_chan_levels calls the batch made.  ask = 0: nobody calls inputLevel().
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "filetuner.h"
#include "gpubatch.h"
#include "radio.h"

static unsigned int bitsOf(float v)
{
	unsigned int u;
	memcpy(&u, &v, sizeof(u));
	return u;
}

int main(int argc, char **argv)
{
	if (argc < 7) {
		fprintf(stderr, "usage: chan_level recording rate block_frames blocks ask if_hz...\n");
		return 2;
	}
	const unsigned int rate = atoi(argv[2]), frames = atoi(argv[3]), blocks = atoi(argv[4]);
	const bool ask = atoi(argv[5]) != 0;
	const size_t R = argc - 6;

	FrontEnd *fe = new FrontEnd(FileTuner::factory);
	Tuner *tuner = fe->tuner();
	tuner->setSubdevice(argv[1]);
	tuner->setSampleRate(rate);
	tuner->setChannels(2);
	tuner->setBlockSize(frames * 2);
	std::vector<Receiver *> rx(R);
	for (size_t r = 0; r < R; r++) {
		rx[r] = new Receiver();                    /* radio.cxx's defaults: 240 kHz channel, 48 kHz audio */
		rx[r]->downconverter()->setIF(atoi(argv[6 + r]));
		rx[r]->demodulator()->setMode(Demodulator::FM);
		rx[r]->setFrontEnd(fe);
	}
	float mean = 0.0f, peak = 0.0f;
	if (!tuner->start()) {
		fprintf(stderr, "start failed\n");
		return 1;
	}
	std::string answers = "[";
	for (unsigned int b = 0; b < blocks; b++) {
		if (!tuner->run()) {
			fprintf(stderr, "run %u failed\n", b);
			return 1;
		}
		answers += b ? ", [" : "[";
		for (size_t r = 0; ask && r < R; r++) {
			mean = peak = 0.0f;
			const bool got = rx[r]->demodulator()->inputLevel(&mean, &peak);
			char text[96];
			snprintf(text, sizeof(text), "%s[%d, %u, %u]", r ? ", " : "", got ? 1 : 0, bitsOf(mean), bitsOf(peak));
			answers += text;
		}
		answers += "]";
	}
	answers += "]";
	printf("{\"answers\": %s, \"block_kernel_calls\": %llu, \"level_calls\": %llu, \"audio_samples\": %lu}\n",
	       answers.c_str(), wr_block_kernel_calls(), wrhost::chanLevelCalls(rx[0]->downconverter()),
	       rx[0]->stream()->totalSamples());
	tuner->stop();
	for (size_t r = 0; r < R; r++)
		delete rx[r];
	delete fe;
	return 0;
}
