"""In how many equal parts a source block goes through the tuner batch (webradio_amd/host/blockparts.h, what
TunerBatch::piecesFor ends with): the arithmetic alone, no GPU.  The rule: as many parts as allowed such that every part
is a whole number of the receivers' common audio period `q` (in source frames) and no shorter than the smallest part."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXXT = os.path.join(ROOT, "tests", "cxx")


@pytest.fixture(scope="module")
def checks():
    lib = os.path.join(CXXT, "libwr_cpu_host_checks.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", CXXT, "libwr_cpu_host_checks.so"])
    L = C.CDLL(lib)
    L.wr_block_parts.restype = C.c_uint
    L.wr_block_parts.argtypes = [C.c_uint, C.c_uint, C.c_ulong, C.c_uint]
    L.wr_lcm_capped.restype = C.c_ulong
    L.wr_lcm_capped.argtypes = [C.c_ulong, C.c_ulong]
    return L


Q = 400 * 1 * 5         # tests/test_gpu_host.py's CFG: 2 Msps -> 5 ksps -> 1 ksps, one audio frame every 2000 source frames


@pytest.mark.parametrize("nframes,pieces,q,smallest,want", [
    (40_000, 4, Q, 1000, 4),            # the three blocks of test_sparse_staging_and_parts_give_the_same_bits:
    (41_000, 4, Q, 1000, 1),            # ... ragged by half an audio frame: no number of parts divides it
    (40_300, 4, Q, 1000, 1),
    (40_000, 4, Q, 500_000, 1),         # the default smallest part: such a block is not worth splitting
    (12_000, 3, Q, 1000, 3),
    (12_000, 4, Q, 1000, 3),            # four parts would be 1.5 audio frames each: the next number down that fits
    (40_000, 4, Q, 10_001, 2),          # ... or that leaves the parts long enough
    (40_000, 4, 0, 1000, 1),            # no common period
    (0, 4, Q, 0, 1),
    (40_000, 1, Q, 1000, 1),
])
def test_parts_of_a_block(checks, nframes, pieces, q, smallest, want):
    assert checks.wr_block_parts(nframes, pieces, q, smallest) == want


def test_lcm_with_a_ceiling(checks):
    assert checks.wr_lcm_capped(6, 4) == 12
    assert checks.wr_lcm_capped(2000, 2000) == 2000
    assert checks.wr_lcm_capped(0, 5) == 0 and checks.wr_lcm_capped(5, 0) == 0
    assert checks.wr_lcm_capped(1 << 40, 1) == 1 << 40                  # the ceiling itself still stands
    assert checks.wr_lcm_capped((1 << 21) + 1, 1 << 21) == 0            # coprime: their lcm is the product, above 2^40
