"""webradio_amd -- MI355X (gfx950) backend for webradio's per-tuner DSP hot path.

The product is the HIP library ``webradio_amd/lib/libwebradio_amd.so`` behind the C ABI
of ``include/webradio_amd.h`` and the C++ host classes in ``webradio_amd/host/`` that keep
the reference's DspBlock operator API.  The Python modules here are plumbing for tests
and bench.py:

  capi    ctypes declarations of the C ABI (fails loudly if the library is not built)
  device  Device / Tuner / Spectrum / ToneBank / DcsBank / Resampler / VoiceBank handles over the C ABI
  synth   synthetic tuner streams (test and bench inputs)
"""
__all__ = ["capi", "device", "synth", "CTCSS_HZ", "DCS_CODES", "DcsBank", "dcs_word", "dcs_step", "Resampler", "resamp_design",
           "resamp_ratio", "DETECTION", "VoiceBank", "voice_design"]


def __getattr__(name):
    # the resampler's, the DCS bank's, the band scan's and the voice bank's names, from device (imported on first use: importing the package loads no library)
    if name in ("Resampler", "resamp_design", "resamp_ratio", "DcsBank", "dcs_word", "dcs_step", "DETECTION", "VoiceBank",
                "voice_design"):
        from . import device
        return getattr(device, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

# the 50 standard CTCSS tones, Hz (device.ToneBank)
CTCSS_HZ = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
            123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
            183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)

# the 104 standard DCS codes (device.DcsBank); written in octal, as they are on a radio's dial
DCS_CODES = (0o023, 0o025, 0o026, 0o031, 0o032, 0o036, 0o043, 0o047, 0o051, 0o053, 0o054, 0o065, 0o071, 0o072, 0o073, 0o074,
             0o114, 0o115, 0o116, 0o122, 0o125, 0o131, 0o132, 0o134, 0o143, 0o145, 0o152, 0o155, 0o156, 0o162, 0o165, 0o172,
             0o174, 0o205, 0o212, 0o223, 0o225, 0o226, 0o243, 0o244, 0o245, 0o246, 0o251, 0o252, 0o255, 0o261, 0o263, 0o265,
             0o266, 0o271, 0o274, 0o306, 0o311, 0o315, 0o325, 0o331, 0o332, 0o343, 0o346, 0o351, 0o356, 0o364, 0o365, 0o371,
             0o411, 0o412, 0o413, 0o423, 0o431, 0o432, 0o445, 0o446, 0o452, 0o454, 0o455, 0o462, 0o464, 0o465, 0o466, 0o503,
             0o506, 0o516, 0o523, 0o526, 0o532, 0o546, 0o565, 0o606, 0o612, 0o624, 0o627, 0o631, 0o632, 0o654, 0o662, 0o664,
             0o703, 0o712, 0o723, 0o731, 0o732, 0o734, 0o743, 0o754)
