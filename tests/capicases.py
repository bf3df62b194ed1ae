"""What the test_*_capi.py modules share: the public header as text, an entry point's declared arguments, the check that it is
declared and bound alike, bit-for-bit equality of float32 arrays and audio with the values a rule treats specially."""
import os
import re

import numpy as np

from webradio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "webradio_amd.h")).read()


def header_args(name):
    """the arguments of `int name(...);` as the header declares them"""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared" % name
    return [a.strip() for a in m.group(1).split(",")]


def declared_and_bound(name, nargs):
    """the header, the binding and the library have `name`, the first two with `nargs` arguments"""
    assert len(header_args(name)) == nargs
    restype, argtypes = capi.SIGNATURES[name]
    assert len(argtypes) == nargs
    assert getattr(capi.load(), name) is not None


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def audio(n, seed, special, max_exp):
    """float32[n]: normal deviates times 10^e, e in [-4, max_exp), both signs -- from 1e-4 to beyond a rule's clamp -- and
    the values of `special` (non-finite, saturating, signed-zero, subnormal ...; none: without them), each twice where n allows"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(n) * 10.0 ** rng.integers(-4, max_exp, n)).astype(np.float32)
    if special:
        where = rng.choice(n, size=min(n, 2 * len(special)), replace=False)
        for k, at in enumerate(where):
            v[at] = np.float32(special[k % len(special)])
    return v
