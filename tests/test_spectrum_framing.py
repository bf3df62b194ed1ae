"""webradio_amd/host/spectrumframing.h: where the reference's most recent complete frame starts inside the last block,
against a walk of the reference's own loop (io/spectrumsink.cxx:101-121), frame by frame from the stream's start.  A
stand-alone g++ program (no GPU, nothing loaded into Python), once plain and once under the address and undefined-behaviour
sanitizers."""
import os

import pytest

import _proc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "webradio_amd", "host")

PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "spectrumframing.h"

/* the reference's loop with a hop: a frame buffer filled from the stream's start, a frame complete whenever fftSize
 * samples lie behind a grid point; `begun` = where the most recent complete frame started, -1 = none yet */
struct Walk {
	unsigned int n, hop;
	long long seen, begun;
	void feed(unsigned long long frames)
	{
		for (unsigned long long i = 0; i < frames; i++) {
			++seen;
			if (seen >= (long long)n && (seen - n) % hop == 0)
				begun = seen - n;
		}
	}
};

int main()
{
	const unsigned int sizes[] = {8, 16}, hops[] = {3, 8, 16, 20};
	unsigned long checked = 0, served = 0;
	for (unsigned int n : sizes)
		for (unsigned int hop : hops)
			for (unsigned int extra = 0; extra < 10; extra++) {
				Walk w = {n, hop, 0, -1};
				unsigned long long total = 0;
				for (unsigned int b = 0; b < 40; b++) {
					/* (submit sizes from n + hop to n + hop + 9, a different one every block) */
					const unsigned long long k = n + hop + (extra + 7u * b) % 10u;
					w.feed(k);
					total += k;
					unsigned long long start = ~0ull;
					const wrhost::SpectrumFrame f = wrhost::spectrumFrameStart(total, n, hop, k, &start);
					++checked;
					if (w.begun < 0) {
						if (f != wrhost::SPECTRUM_FRAME_NONE)
							return printf("n %u hop %u block %u: a frame before the walk has one\n", n, hop, b), 1;
						continue;
					}
					if (f != wrhost::SPECTRUM_FRAME_AT || (long long)(total - k + start) != w.begun || start + n > k)
						return printf("n %u hop %u block %u: %d start %llu, the walk's frame begins at %lld of %llu (k %llu)\n", n,
						              hop, b, (int)f, start, w.begun, total, k), 1;
					++served;
				}
			}
	/* hop 0 is the reference: back to back */
	unsigned long long start = 0;
	if (wrhost::spectrumFrameStart(40, 16, 0, 33, &start) != wrhost::SPECTRUM_FRAME_AT || start != 16 - 7)
		return printf("hop 0\n"), 1;
	if (wrhost::spectrumFrameStart(15, 16, 0, 15, &start) != wrhost::SPECTRUM_FRAME_NONE)
		return printf("none yet\n"), 1;
	/* a last block too short to hold the frame is reported, not served */
	if (wrhost::spectrumFrameStart(100, 16, 16, 3, &start) != wrhost::SPECTRUM_FRAME_OUTSIDE)
		return printf("outside\n"), 1;
	printf("checked %lu served %lu\n", checked, served);
	return 0;
}
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_frame_start_is_the_reference_walk_s(tmp_path, flags):
    assert os.path.exists(os.path.join(HOST, "spectrumframing.h"))
    src = tmp_path / "framing.cxx"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "framing")
    _proc.run(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Werror", "-I" + HOST] + flags + [str(src), "-o", exe], timeout=120)
    out = _proc.output([exe], timeout=60).decode()
    print(out)
    assert out.startswith("checked 3200 served")
    assert int(out.split()[3]) >= 3000
