/*
 * spec_avg_plan.cxx -- wr_spectrum_batch_avg's plan (webradio_amd/csrc/wr_plan.h) behind a C interface, for
 * tests/test_spectrum_avg_reference.py, which compiles it with the host compiler and loads it with ctypes.  No HIP.
 */
#include "wr_plan.h"

extern "C" {

size_t spec_avg_cap_bytes(void)
{
	return SPEC_AVG_BYTES;
}

/* fchunk, gchunk, carry and the scratch bytes of a call */
void spec_avg_plan(unsigned int n, size_t F, size_t G, size_t *out4)
{
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	out4[0] = p.fchunk;
	out4[1] = p.gchunk;
	out4[2] = p.carry;
	out4[3] = wrp_spec_avg_bytes(n, p);
}

/* the call's chunks in the order the library walks them, `max` at most: rows of (g0, ng, f0, nf); returns how many there are */
size_t spec_avg_chunks(unsigned int n, size_t F, size_t G, size_t max, size_t *rows)
{
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	WrSpecAvgChunk c;
	size_t count = 0;
	for (bool more = wrp_spec_avg_next(p, F, G, &c, true); more; more = wrp_spec_avg_next(p, F, G, &c, false)) {
		if (count < max) {
			rows[4 * count] = c.g0;
			rows[4 * count + 1] = c.ng;
			rows[4 * count + 2] = c.f0;
			rows[4 * count + 3] = c.nf;
		}
		++count;
		if (count > max)
			break;
	}
	return count;
}

/* path (WrFftPath) of a spectrum */
int spec_avg_path(unsigned int n, unsigned int channels)
{
	return (int)wrp_fft_shape(n, channels).path;
}

/* launches of a call whose plan's work area holds what a call for its chunk reserves */
size_t spec_avg_launches(unsigned int n, unsigned int channels, size_t F, size_t G)
{
	const WrSpecAvgPlan p = wrp_spec_avg_plan(n, F, G);
	return wrp_spec_avg_launches(n, channels, F, G, wrp_fft_work_frames(n, 1, p.fchunk));
}

unsigned int spec_avg_reduce_grid(unsigned int n, size_t ng)
{
	return wrp_spec_reduce_grid(n, ng);
}

}
