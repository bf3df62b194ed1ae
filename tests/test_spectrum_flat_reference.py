"""oracle.spectrum_np -- the fast reference of the all-bins spectrum tests (tests/test_gpu_spectrum_all_bins.py) -- held
to oracle.Spectrum on every bin, and the condition that keeps those tests' dB mask honest: on the flat input the mask
leaves out at most MASK_OUT_SHARE of a frame's bins.  No GPU."""
import numpy as np
import pytest

import wr_oracle as oracle
from flat_spectrum import MASK_OUT_SHARE, db_error, flat, interleaved, left_out

SIZES = [1 << b for b in range(3, 21)]


@pytest.mark.parametrize("n", [8, 512, 65536, 1 << 20])
def test_fast_reference_is_the_oracle_s(n):
    """Bins within 1e-7 * peak on EVERY bin (the oracle's are rounded to float32: 6e-8 of a bin's own size), dB within
    1e-4 dB on the masked bins (the oracle's is the reference's float32 expression)."""
    iq = flat(2 * n, seed=n)
    o = oracle.Spectrum(n)
    o.process(iq)
    assert o.frames_done == 1
    want_db, want_bins = oracle.spectrum_np(iq.view(np.complex64))
    peak = np.abs(want_bins).max()
    err = float(np.abs(o.bins().astype(np.float64) - interleaved(want_bins)).max())
    db_err, out = db_error(o.get().astype(np.float64), want_db)
    print("n=%d oracle against numpy: bins %.3g x peak, dB %.3g on %d of %d bins" % (n, err / peak, db_err, n - out, n))
    assert err <= 1e-7 * peak
    assert db_err <= 1e-4


def test_fast_reference_of_real_frames_is_that_of_x_0():
    n = 4096
    x = flat(n, seed=5)
    z = np.zeros(n, np.complex64)
    z.real = x
    a, b = oracle.spectrum_np(x), oracle.spectrum_np(z)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    rows = oracle.spectrum_np(np.stack([z, z[::-1]]))
    assert np.array_equal(rows[0][0], b[0]) and np.array_equal(rows[1][0], b[1])


@pytest.mark.parametrize("n", SIZES)
def test_mask_keeps_nearly_every_bin_of_the_flat_input(n):
    """With the reference alone: 0 bins left out up to 32768, 1 at 65536, about a dozen of 1048576."""
    for what, frame in (("IQ", flat(2 * n, seed=n).view(np.complex64)), ("real", flat(n, seed=n + 1))):
        want_db = oracle.spectrum_np(frame)[0]
        out = int(left_out(want_db)[0])
        print("n=%d %s: the mask leaves out %d bins" % (n, what, out))
        assert out <= MASK_OUT_SHARE * n
