"""What the spectrum tests share, GPU and CPU-only alike (numpy only: importing it loads no library).

Tolerance: the reference runs FFTW's float transform, the oracle a double-accumulated one, the GPU a float32 radix-2
Stockham.  Complex bins agree within BIN_RTOL * max|X| (float32 butterfly rounding grows ~ log2 N); dB values are compared
on the bins within 60 dB of the frame's peak with DB_ATOL (below that a bin is rounding noise over rounding noise)."""
import numpy as np

BIN_RTOL = 2e-6
DB_ATOL = 0.02


def db_error(got_db, want_db):
    """the strong-bins rule: the largest dB difference on the bins within 60 dB of the wanted row's peak"""
    assert got_db.shape == want_db.shape, "a dB row of shape %s against one of %s" % (got_db.shape, want_db.shape)
    strong = want_db >= want_db.max() - 60.0
    return float(np.abs(got_db[strong] - want_db[strong]).max())


def check_db(got_db, want_db, what=""):
    """db_error within DB_ATOL; prints the figure it then asserts on"""
    err = db_error(got_db, want_db)
    print("%s n=%d dB error on strong bins %.3g (bound %.3g)" % (what, want_db.size, err, DB_ATOL))
    assert err <= DB_ATOL, "%s n=%d: dB error on strong bins %.6g, bound %.6g" % (what, want_db.size, err, DB_ATOL)
