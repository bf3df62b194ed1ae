"""The C ABI of the spectrum of real samples (wr_spectrum_create_real, wr_spectrum_channels, wr_spectrum_batch_db_rows):
declared, exported, bound, and refusing bad arguments.  No GPU needed (and none used)."""
import ctypes as C
import re

import capicases
from webradio_amd import capi

NEW = ("wr_spectrum_create_real", "wr_spectrum_channels", "wr_spectrum_batch_db_rows")


def test_header_library_and_binding_have_the_new_functions():
    code = re.sub(r"/\*.*?\*/", "", capicases.header(), flags=re.S)
    lib = capi.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
        assert capi.SIGNATURES[name][0] is C.c_int


def test_abi_version_is_still_6():
    assert capi.load().wr_abi_version() == capi.WR_ABI_VERSION == 6
    assert re.search(r"#define\s+WR_ABI_VERSION\s+6\b", capicases.header())


def test_null_handles_are_refused_with_a_message():
    lib = capi.load()
    assert lib.wr_spectrum_create_real(None, None, 512, 0) == capi.WR_ERR_ARG
    assert b"wr_spectrum_create_real" in lib.wr_last_error()
    assert lib.wr_spectrum_batch_db_rows(None, None, 512, 1, None) == capi.WR_ERR_ARG
    assert b"wr_spectrum_batch_db_rows" in lib.wr_last_error()
    ch = C.c_uint(7)
    assert lib.wr_spectrum_channels(None, C.byref(ch)) == capi.WR_ERR_ARG
    assert b"wr_spectrum_channels" in lib.wr_last_error()
    assert ch.value == 7


def test_header_cites_the_reference_s_fixmes():
    assert "io/spectrumsink.cxx:62-64" in capicases.header()
