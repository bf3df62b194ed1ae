/*
 * wr_design.cpp -- host-side, one-off design math of the backend: NCO tables,
 * phase step, FIR tap design, windows, FFT twiddles.  None of this is per-sample
 * work; the reference does the same things once in constructors / init() /
 * setters and so do we, on the host, then upload.
 *
 * Reference paths are relative to webradio's src/.
 */
#include "wr_internal.h"

#include <cmath>
#include <cstring>

namespace {
const double kPi = 3.14159265358979323846;   /* the value of M_PI the reference compiles in */
}

/* The DownConverter constructor's table (dsp/downconverter.cxx:49-51).  The kernels in
 * WR_NCO_EXACT mode gather from exactly this table, so it is produced the way the
 * reference produces it: float index doubled in float, scaled by M_PI/65536 in double,
 * narrowed, then libm sinf. */
void wrd_sin_table(float *table)
{
	const float entries = (float)WR_TABLE_SIZE;
	for (unsigned int n = 0; n < WR_TABLE_SIZE; ++n) {
		float twice = (float)n * 2;
		double angle = twice * kPi / entries;
		table[n] = sinf((float)angle);
	}
}

/* DownConverter::init / setIF (dsp/downconverter.cxx:65,80): signed 64-bit
 * hz * 2^31 / rate, C++ division (truncates toward zero), narrowed to int. */
/* sin(2 pi n / 65536) evaluated in double on the exact angle and narrowed once: the turns of
 * WR_NCO_ROTATE.  (The reference's table above carries the rounding of its float ARGUMENT, up
 * to 2.4e-7 per entry: harmless for one lookup, but a turn is applied up to 15 times in a row,
 * and |turn| != 1 compounds.) */
void wrd_sin_table_rounded(float *table)
{
	for (unsigned int n = 0; n < WR_TABLE_SIZE; ++n) {
		/* exact octant reduction keeps the symmetry sin^2 + cos^2 = 1 to the last bit of double */
		table[n] = (float)sin(2.0 * kPi * (double)n / (double)WR_TABLE_SIZE);
	}
	table[0] = 0.0f;
	table[WR_TABLE_SIZE / 2] = 0.0f;                       /* sin(pi): exactly zero, not 1.2e-16 */
}

int wrd_phase_step(int if_hz, unsigned int input_rate)
{
	long long num = (long long)if_hz * (1LL << 31);
	return (int)(num / (long long)input_rate);
}

/* dsp/lowpass.cxx:167 -- 32-bit unsigned arithmetic, evaluated left to right, so the
 * product wraps for passbands above 2^32/64 Hz and narrow passbands give bin 0. */
unsigned wrd_lowpass_maxbin(unsigned int L, unsigned int passband, unsigned int input_rate)
{
	unsigned int scaled = L * passband;               /* wraps modulo 2^32 like lowpass.cxx:167 */
	return scaled / input_rate / 2u;
}

/* LowPass::init window (dsp/lowpass.cxx:104-110) and LowPass::recalculate
 * (dsp/lowpass.cxx:164-189).
 *
 * The reference fills an L-bin real, even spectrum (L = _firLength, 64 as compiled) with ones
 * below `maxbin`, runs an unnormalised inverse DFT and keeps Re(impulse[(n+L/2)&(L-1)]) *
 * window[n].  For that 0/1 even spectrum the inverse DFT has the closed form of a Dirichlet
 * kernel,
 *      impulse[m] = e0 + 2*sum_{b=1}^{maxbin-1} cos(2*pi*b*m/L)      (+ Nyquist term)
 * which is what is evaluated here (in double, narrowed once).  Bins run to L/2 inclusive
 * (lowpass.cxx:173), so maxbin = L/2+1 would also switch the Nyquist bin on.  L is a power of
 * two (the mask logic of lowpass.cxx:172,184). */
void wrd_lowpass_design(unsigned int L, unsigned int passband, unsigned int input_rate, float *coeff)
{
	const unsigned int maxbin = wrd_lowpass_maxbin(L, passband, input_rate);

	for (unsigned int n = 0; n < L; ++n) {
		/* window sample, float arithmetic where the reference's is float */
		double warg = 2 * kPi * (double)(float)n / (double)(float)(L - 1);
		float w = (float)(0.54 - 0.46 * (double)cosf((float)warg));
		w /= (float)L;

		unsigned int m = (n + L / 2) & (L - 1);
		double acc = 0.0;
		if (maxbin > 0)
			acc += 1.0;                                   /* bin 0 */
		for (unsigned int b = 1; b < maxbin && b < L / 2; ++b) {
			unsigned int turn = (b * m) & (L - 1);        /* exact reduction of b*m/L turns */
			acc += 2.0 * cos(2.0 * kPi * (double)turn / (double)L);
		}
		if (maxbin > L / 2)                               /* bin L/2 switched on */
			acc += (m & 1u) ? -1.0 : 1.0;
		coeff[n] = (float)acc * w;
	}
}

/* SpectrumSink::init (io/spectrumsink.cxx:71-74): plain Hamming, no 1/N. */
void wrd_spectrum_window(unsigned int n, float *window)
{
	const float last = (float)(n - 1);
	for (unsigned int k = 0; k < n; ++k) {
		double arg = 2 * kPi * (double)(float)k / (double)last;
		window[k] = (float)(0.54 - 0.46 * (double)cosf((float)arg));
	}
}

/* WR_NCO_SPLIT tables.  The table index idx = phase >> 15 (16 bits) is split into a
 * coarse byte a and a fine byte b; sin/cos(2*pi*idx/65536) follow from the angle
 * addition of hi[a] = cis(2*pi*a/256) and lo[b] = cis(2*pi*b/65536). */
void wrd_split_tables(float *hi_cs, float *lo_cs)
{
	for (unsigned int k = 0; k < WR_SPLIT_N; ++k) {
		double ah = 2.0 * kPi * (double)k / 256.0;
		double al = 2.0 * kPi * (double)k / 65536.0;
		hi_cs[2 * k] = (float)cos(ah);
		hi_cs[2 * k + 1] = (float)sin(ah);
		lo_cs[2 * k] = (float)cos(al);
		lo_cs[2 * k + 1] = (float)sin(al);
	}
}

/* forward-transform twiddles exp(-2*pi*i*k/n), k < n/2, as (cos, -sin) pairs */
void wrd_twiddles(unsigned int n, float *tw)
{
	for (unsigned int k = 0; k < n / 2; ++k) {
		double a = 2.0 * kPi * (double)k / (double)n;
		tw[2 * k] = (float)cos(a);
		tw[2 * k + 1] = (float)(-sin(a));
	}
}

/* wr_agc_design (include/webradio_amd.h): the three numbers of a receiver's AGC from its settings in dB.  The envelope
 * lives in the bit pattern of a float, where an octave -- 20 log10(2) = 6.02 dB of amplitude -- is 2^23 units. */
int wrd_agc_design(float target_dbfs, float decay_db_per_s, float max_gain_db, unsigned int audio_rate, float *target,
                   unsigned int *floor_bits, unsigned int *step)
{
	if (!(target_dbfs >= -100.0f && target_dbfs <= 0.0f) || !(decay_db_per_s >= 0.0f && decay_db_per_s <= 1.0e4f) ||
	    !(max_gain_db >= 0.0f && max_gain_db <= 120.0f) || !audio_rate)
		return 1;                                               /* (a NaN fails every comparison) */
	const double level = pow(10.0, (double)target_dbfs / 20.0);
	const float floor_f = (float)(level / pow(10.0, (double)max_gain_db / 20.0));
	if (!(floor_f >= 1.17549435e-38f))
		return 1;
	const double per_frame = (double)decay_db_per_s / (20.0 * log10(2.0)) * 8388608.0 / (double)audio_rate;
	const long long units = llround(per_frame);
	*target = (float)level;
	memcpy(floor_bits, &floor_f, sizeof(*floor_bits));
	*step = units > 0x80000000ll ? 0x80000000u : (unsigned int)units;
	return 0;
}

/* wr_tone_step (include/webradio_amd.h): a tone's phase step per audio frame, in units of 2^-32 of a turn */
int wrd_tone_step(double hz, unsigned int audio_rate, unsigned int *step)
{
	if (!audio_rate || !(hz > 0.0) || !(hz < (double)audio_rate / 2.0))       /* (a NaN fails every comparison) */
		return 1;
	*step = (unsigned int)llround(hz / (double)audio_rate * 4294967296.0);
	return 0;
}

/* wr_resamp_ratio (include/webradio_amd.h): both rates divided by their gcd */
int wrd_resamp_ratio(unsigned int in_rate, unsigned int out_rate, unsigned int *L, unsigned int *M)
{
	if (!in_rate || !out_rate)
		return 1;
	unsigned int a = in_rate, b = out_rate;
	while (b) {
		const unsigned int r = a % b;
		a = b;
		b = r;
	}
	*L = out_rate / a;
	*M = in_rate / a;
	return 0;
}

/* the header's limits on a resampler's ratio and taps per phase */
int wrd_resamp_limits(unsigned int L, unsigned int M, unsigned int P)
{
	return wrp_resamp_limits_bad(L, M, P);
}

namespace {
/* the modified Bessel function I0 by its power series: sum ((x / 2)^k / k!)^2, terms falling from k > x / 2 on */
double bessel_i0(double x)
{
	const double q = x * x / 4.0;
	double term = 1.0, sum = 1.0;
	for (unsigned int k = 1; k < 500u; ++k) {
		term *= q / ((double)k * (double)k);
		sum += term;
		if (term < sum * 1e-18)
			break;
	}
	return sum;
}
}

/* wr_resamp_design (include/webradio_amd.h): the Kaiser-windowed sinc, in double, narrowed once; taps[L][P].  Non-zero: a
 * limit, or no passband */
int wrd_resamp_design(unsigned int in_rate, unsigned int out_rate, unsigned int P, float *taps, unsigned int *L_out,
                      unsigned int *M_out)
{
	unsigned int L, M;
	if (wrd_resamp_ratio(in_rate, out_rate, &L, &M) || wrd_resamp_limits(L, M, P))
		return 1;
	const unsigned int lo = in_rate < out_rate ? in_rate : out_rate;
	if (!((unsigned long long)lo * P > 10ull * in_rate))
		return 1;
	const double beta = 8.0, width = 5.0 * (double)in_rate / (double)P;
	const double fc = (double)lo / 2.0 - width / 2.0;
	const double wn = 2.0 * fc / ((double)L * (double)in_rate);            /* cut-off in units of the Nyquist rate at L x in_rate */
	const unsigned int nh = L * P;
	const double mid = ((double)nh - 1.0) / 2.0, i0b = bessel_i0(beta);
	double *h = new double[nh];
	double sum = 0.0;
	for (unsigned int i = 0; i < nh; ++i) {
		const double x = wn * ((double)i - mid);
		const double s = x == 0.0 ? 1.0 : sin(kPi * x) / (kPi * x);
		const double u = ((double)i - mid) / mid;
		const double w = bessel_i0(beta * sqrt(1.0 - u * u > 0.0 ? 1.0 - u * u : 0.0)) / i0b;
		h[i] = s * w;
		sum += h[i];
	}
	for (unsigned int k = 0; k < P; ++k)
		for (unsigned int ph = 0; ph < L; ++ph)
			taps[(size_t)ph * P + k] = (float)(h[(size_t)k * L + ph] * (double)L / sum);
	delete[] h;
	*L_out = L;
	*M_out = M;
	return 0;
}

/* wr_voice_design (include/webradio_amd.h): the frequency-sampled band-pass with de-emphasis under a Kaiser window, in
 * double, narrowed once; taps[T] with taps[T - 1] = +0.  The grid has G = 32768 points, so the turn g (i - d) / G is
 * reduced exactly (mod G, in integers) and the cosine comes from one table of G entries.  The upper half of the N = T - 1
 * taps is the mirror of the lower one: the same bits.  Non-zero: a limit, or edges too close for the window */
int wrd_voice_design(unsigned int audio_rate, unsigned int T, unsigned int highpass_hz, unsigned int lowpass_hz,
                     unsigned int deemph_us, float *taps)
{
	const unsigned int G = 32768u;
	const double beta = 6.0;
	if (!audio_rate || !wrp_voice_len_ok(T) || deemph_us > 10000u)
		return 1;
	const double rate = (double)audio_rate;
	if (lowpass_hz && 2.0 * (double)lowpass_hz >= rate)
		return 1;
	if (highpass_hz && 2.0 * (double)highpass_hz >= rate)          /* (nothing would be left of the band) */
		return 1;
	const double W = (beta / 0.1102 + 8.7 - 8.0) / (2.285 * 2.0 * kPi * ((double)T - 1.0)) * rate;
	if (highpass_hz && lowpass_hz && (double)highpass_hz + W >= (double)lowpass_hz - W)
		return 1;
	const unsigned int N = T - 1u, d = T / 2u - 1u;
	const double tau = (double)deemph_us * 1e-6;
	const double de1k = 1.0 + (2.0 * kPi * 1000.0 * tau) * (2.0 * kPi * 1000.0 * tau);
	double *D = new double[G / 2u + 1u];
	double *cs = new double[G];
	unsigned int g_lo = G, g_hi = 0;                              /* the grid points where D is not 0 */
	for (unsigned int g = 0; g <= G / 2u; ++g) {
		const double f = (double)g * rate / (double)G;
		const bool band = (!highpass_hz || f >= (double)highpass_hz) && (!lowpass_hz || f <= (double)lowpass_hz);
		const double w = 2.0 * kPi * f * tau;
		D[g] = !band ? 0.0 : !deemph_us ? 1.0 : sqrt(de1k / (1.0 + w * w));
		if (band) {
			if (g < g_lo)
				g_lo = g;
			g_hi = g;
		}
	}
	for (unsigned int q = 0; q < G; ++q)
		cs[q] = cos(2.0 * kPi * (double)q / (double)G);
	cs[G / 4u] = cs[3u * G / 4u] = 0.0;                           /* cos(pi / 2): exactly zero, not 6e-17 */
	const double i0b = bessel_i0(beta);
	for (unsigned int i = 0; i <= d; ++i) {
		const unsigned int m = d - i;                                 /* |i - d|: the cosine is even */
		double acc = 0.0;
		for (unsigned int g = g_lo; g <= g_hi && g_lo <= g_hi; ++g) {
			const double term = D[g] * cs[(unsigned int)(((unsigned long long)g * m) & (G - 1u))];
			acc += (g == 0 || g == G / 2u) ? term : 2.0 * term;
		}
		const double u = 2.0 * (double)i / ((double)N - 1.0) - 1.0;
		const double win = bessel_i0(beta * sqrt(1.0 - u * u > 0.0 ? 1.0 - u * u : 0.0)) / i0b;
		taps[i] = taps[N - 1u - i] = (float)(acc / (double)G * win);
	}
	taps[T - 1u] = 0.0f;
	delete[] D;
	delete[] cs;
	return 0;
}
