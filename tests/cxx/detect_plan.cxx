/*
 * detect_plan.cxx -- wr_spectrum_rows_detect's plan (webradio_amd/csrc/wr_plan.h) behind a C interface, for
 * tests/test_detect_reference.py, which compiles it with the host compiler and loads it with ctypes.  No HIP.
 */
#include "wr_plan.h"

extern "C" {

/* threads, bins of a tile, keys the LDS holds, the cap of a chunk's floors, what a workgroup may have of LDS */
void detect_constants(size_t *out5)
{
	out5[0] = DETECT_THREADS;
	out5[1] = DETECT_TILE;
	out5[2] = DETECT_LDS_KEYS;
	out5[3] = DETECT_FLOOR_BYTES;
	out5[4] = DETECT_WG_LDS_MAX;
}

/* the field that breaks a limit, or NULL */
const char *detect_rule_bad(unsigned int n, const wr_detect_rule *rule)
{
	return wrp_detect_rule_bad(n, rule);
}

/* nspans, chunk_rows, floor_bytes, keys_in_lds, lds_floor, lds_segments of a call with a valid rule */
void detect_plan(const wr_detect_rule *rule, size_t nrows, size_t *out6)
{
	const WrDetectPlan p = wrp_detect_plan(rule, nrows);
	out6[0] = p.nspans;
	out6[1] = p.chunk_rows;
	out6[2] = p.floor_bytes;
	out6[3] = p.keys_in_lds;
	out6[4] = p.lds_floor;
	out6[5] = p.lds_segments;
}

/* the call's chunks in the order the library walks them, `max` at most: rows of (r0, nr, floor grid, segments grid); returns
 * how many there are */
size_t detect_chunks(const wr_detect_rule *rule, size_t nrows, size_t max, size_t *rows)
{
	const WrDetectPlan p = wrp_detect_plan(rule, nrows);
	size_t r0 = 0, nr = 0, count = 0;
	for (bool more = wrp_detect_next(p, nrows, &r0, &nr, true); more; more = wrp_detect_next(p, nrows, &r0, &nr, false)) {
		if (count < max) {
			rows[4 * count] = r0;
			rows[4 * count + 1] = nr;
			rows[4 * count + 2] = wrp_detect_floor_grid(p, nr);
			rows[4 * count + 3] = wrp_detect_segments_grid(nr);
		}
		++count;
		if (count > max)
			break;
	}
	return count;
}

}
