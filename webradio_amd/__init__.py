"""webradio_amd -- MI355X (gfx950) backend for webradio's per-tuner DSP hot path.

The product is the HIP library ``webradio_amd/lib/libwebradio_amd.so`` behind the C ABI
of ``include/webradio_amd.h`` and the C++ host classes in ``webradio_amd/host/`` that keep
the reference's DspBlock operator API.  The Python modules here are plumbing for tests
and bench.py:

  capi    ctypes declarations of the C ABI (fails loudly if the library is not built)
  device  Device / Tuner / Spectrum / ToneBank / Resampler handles over the C ABI
  synth   synthetic tuner streams (test and bench inputs)
"""
__all__ = ["capi", "device", "synth", "CTCSS_HZ", "Resampler", "resamp_design", "resamp_ratio"]


def __getattr__(name):
    # the resampler's names, from device (imported on first use: importing the package loads no library)
    if name in ("Resampler", "resamp_design", "resamp_ratio"):
        from . import device
        return getattr(device, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

# the 50 standard CTCSS tones, Hz (device.ToneBank)
CTCSS_HZ = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
            123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
            183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
