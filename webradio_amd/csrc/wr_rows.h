/*
 * wr_rows.h -- what the row kernels (wr_tones.hip, wr_dcs.hip, wr_resamp.hip, wr_voice.hip) do to an audio value before
 * anything else, in one copy.  Device code only.
 */
#ifndef WR_ROWS_H_
#define WR_ROWS_H_

/* x' of the filters' rules: 0 for an inf or a NaN, else x within +-65536 */
__device__ __forceinline__ float row_clean(float x)
{
	if ((__float_as_uint(x) & 0x7fffffffu) >= 0x7f800000u)
		x = 0.0f;
	return fminf(fmaxf(x, -65536.0f), 65536.0f);
}

/* w of the correlators' rules: 0 for an inf or a NaN, else v within +-64, times 2^24 -- |w| <= 2^30, rint(w) fits an int */
__device__ __forceinline__ float row_fixed24(float v)
{
	if ((__float_as_uint(v) & 0x7fffffffu) >= 0x7f800000u)
		v = 0.0f;
	return fminf(fmaxf(v, -64.0f), 64.0f) * 16777216.0f;
}

#endif
