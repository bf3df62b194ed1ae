/*
 * spectrumframing.h -- WHICH frame a SpectrumSink shows, for a sink that is served out of the last block its producer
 * delivered and keeps no samples of its own (a sink on a Receiver's channel filter inside the tuner batch, gpubatch.h).
 *
 * The reference fills its frame buffer from the stream's start and transforms whenever it is full
 * (io/spectrumsink.cxx:101-121): frames lie on a grid from the first sample, and getSpectrum() shows the most recent
 * COMPLETE one.  With this backend's hop (frames start every `hop` input frames, 0 = back to back = the reference) that is
 * the frame that starts at s = ((total - n) / hop) * hop once `total` >= n frames have been delivered.  Since
 * total - s < n + hop, a last block of k >= n + hop frames holds that frame whole.  No GPU code here.
 */
#ifndef WRHOST_SPECTRUMFRAMING_H_
#define WRHOST_SPECTRUMFRAMING_H_

namespace wrhost {

enum SpectrumFrame {
	SPECTRUM_FRAME_NONE = 0,        /* fewer than n frames so far: no complete frame yet */
	SPECTRUM_FRAME_AT = 1,          /* *start = where it begins, in frames from the start of the last block */
	SPECTRUM_FRAME_OUTSIDE = -1     /* it begins before the last block (k < n + hop): it cannot be served from there */
};

/* total: frames delivered so far, the last block's k among them; n: the transform size; hop: 0 = n */
static inline SpectrumFrame spectrumFrameStart(unsigned long long total, unsigned int n, unsigned int hop,
                                               unsigned long long k, unsigned long long *start)
{
	if (!hop)
		hop = n;
	if (!n || total < n || k > total)
		return k > total ? SPECTRUM_FRAME_OUTSIDE : SPECTRUM_FRAME_NONE;
	const unsigned long long s = ((total - n) / hop) * hop;     /* from the stream's start */
	const unsigned long long base = total - k;                  /* ... where the last block begins */
	if (s < base)
		return SPECTRUM_FRAME_OUTSIDE;
	*start = s - base;                                          /* (s + n <= total: it ends inside the block too) */
	return SPECTRUM_FRAME_AT;
}

} // namespace wrhost

#endif /* WRHOST_SPECTRUMFRAMING_H_ */
