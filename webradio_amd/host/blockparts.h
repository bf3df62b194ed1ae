/*
 * blockparts.h -- in how many equal parts a source block goes through the tuner batch (TunerBatch::piecesFor): the
 * arithmetic alone, with no GPU call and no environment read, so that a CPU test can hold it to the rule.
 */
#ifndef WRHOST_BLOCKPARTS_H_
#define WRHOST_BLOCKPARTS_H_

namespace wrhost {

/* lcm with a ceiling: anything this large stands for "do not split" */
inline unsigned long lcmCapped(unsigned long a, unsigned long b)
{
	if (!a || !b)
		return 0;
	unsigned long x = a, y = b;
	while (y) {
		const unsigned long t = x % y;
		x = y;
		y = t;
	}
	const unsigned long long l = (unsigned long long)(a / x) * b;
	return l > (1ull << 40) ? 0 : (unsigned long)l;
}

/* The most parts, `pieces` at the most, such that every part of a block of `nframes` is a whole number of `q` frames -- the
 * common period of the receivers' audio frames, in source frames -- and no shorter than `minFrames`.  1: do not split
 * (q = 0: the periods have no common one worth having) */
inline unsigned int partsOf(unsigned int nframes, unsigned int pieces, unsigned long q, unsigned int minFrames)
{
	if (!nframes || !q)
		return 1;
	for (unsigned int p = pieces; p > 1; p--)
		if (nframes % (p * q) == 0 && nframes / p >= minFrames)
			return p;
	return 1;
}

} // namespace wrhost

#endif /* WRHOST_BLOCKPARTS_H_ */
