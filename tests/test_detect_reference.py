"""wr_spectrum_rows_detect without a GPU: the calls exist and refuse bad arguments, the host-side helpers give their values,
the two statements of the rule (tests/detect_np.py) agree with each other and with known answers, the planted streams of
tests/test_gpu_detect.py keep their margin on the reference alone, and the plan of a call (webradio_amd/csrc/wr_plan.h)
keeps its promises."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import detect_np as dn
import launch_plan
import specavg_np as sa
from flat_spectrum import MASK_OUT_SHARE
from speccases import DB_ATOL
from webradio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wr_detect_rule_default", "wr_spectrum_bin_hz", "wr_spectrum_rows_detect")


@pytest.fixture(autouse=True)
def _the_calls_exist():
    """this module's statements of the rule and its plan are those of the three calls: without them in the library and the
    binding nothing here means anything"""
    lib = capi.load()
    for name in NEW:
        assert name in capi.SIGNATURES and hasattr(lib, name), name


def test_the_names_are_in_the_library_the_binding_and_the_package():
    import webradio_amd
    from webradio_amd import device
    assert webradio_amd.DETECTION == dn.DETECTION and webradio_amd.DETECTION.itemsize == 24
    assert C.sizeof(capi.DetectRule) == 32 and [f for f, _ in capi.DetectRule._fields_] == list(dn.FIELDS)
    for name in ("rows_detect", "detect", "bin_hz"):
        assert hasattr(device.Spectrum, name)
    text = open(os.path.join(ROOT, "include", "webradio_amd.h")).read()
    assert "Added to 6 later: wr_detect_rule_default, wr_spectrum_bin_hz, wr_spectrum_rows_detect." in text


def test_the_abi_version_stays():
    assert capi.load().wr_abi_version() == capi.WR_ABI_VERSION == 6


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()
    rule = capi.DetectRule()
    one = C.c_uint()
    for spec, r, count in ((None, C.byref(rule), C.byref(one)), (None, None, C.byref(one)), (None, C.byref(rule), None)):
        assert lib.wr_spectrum_rows_detect(spec, None, 0, r, 0, None, count, None) == capi.WR_ERR_ARG
        assert b"wr_spectrum_rows_detect" in lib.wr_last_error()
    assert lib.wr_detect_rule_default(512, None) == capi.WR_ERR_ARG
    assert b"wr_detect_rule_default" in lib.wr_last_error()
    for bad in (0, 4, 12, 1000, 1 << 21):
        assert lib.wr_detect_rule_default(bad, C.byref(rule)) == capi.WR_ERR_ARG
        assert b"wr_detect_rule_default" in lib.wr_last_error()
    hz = C.c_double()
    for n, rate, out in ((512, 48000, None), (512, 0, C.byref(hz)), (500, 48000, C.byref(hz)), (4, 48000, C.byref(hz))):
        assert lib.wr_spectrum_bin_hz(n, rate, 0.0, 1.0, out) == capi.WR_ERR_ARG
        assert b"wr_spectrum_bin_hz" in lib.wr_last_error()


@pytest.mark.parametrize("n", [8, 512, 1024, 4096, 1 << 20])
def test_the_default_rule(n):
    rule = capi.DetectRule()
    assert capi.load().wr_detect_rule_default(n, C.byref(rule)) == capi.WR_OK
    got = {f: getattr(rule, f) for f in dn.FIELDS}
    assert got == dict(bin0=0, nbins=n, span=min(n, 1024), percent=50, threshold=10.0, linear=0, max_gap=1, min_width=1)
    assert got == dn.rule_of(n)


def test_bin_hz():
    """DC sits at n / 2; the first bin is half the rate below the centre, the last one bin short of half the rate above
    it; a half bin is half a bin's width (all exact in double at these values)"""
    from webradio_amd.device import bin_hz
    n, rate, centre = 4096, 2_048_000, 100e6
    assert bin_hz(n, rate, centre, n / 2) == centre
    assert bin_hz(n, rate, centre, 0) == centre - rate / 2
    assert bin_hz(n, rate, centre, n - 1) == centre + rate / 2 - rate / n
    assert bin_hz(n, rate, centre, n / 2 + 0.5) == centre + 0.5 * rate / n
    assert bin_hz(8, 48000, 0.0, (2 + 5) / 2) == -0.5 * 6000.0
    assert abs(bin_hz(1 << 20, 100_000_000, 0.0, (1 << 19) + 3) - 3 * 100e6 / (1 << 20)) <= 1e-9


# ---- the rule's limits and the plan ------------------------------------------------------------------------------------------

SIZE = C.c_size_t


@pytest.fixture(scope="module")
def plan():
    return launch_plan.lib()


def _constants(lib):
    out = (SIZE * 5)()
    lib.detect_constants(out)
    return dict(zip(("threads", "tile", "lds_keys", "floor_bytes", "lds_max"), out))


def _plan(lib, rule, nrows):
    out = (SIZE * 6)()
    lib.detect_plan(C.byref(capi.DetectRule(**rule)), nrows, out)
    return dict(zip(("nspans", "chunk_rows", "floor_bytes", "keys_in_lds", "lds_floor", "lds_segments"), out))


def test_the_rule_s_limits(plan):
    n = 4096

    def bad(**fields):
        got = plan.detect_rule_bad(n, C.byref(capi.DetectRule(**dn.rule_of(n, **fields))))
        return got.decode() if got else None

    assert bad() is None
    assert bad(bin0=96, nbins=4000, span=8) is None and bad(bin0=n - 8, nbins=8, span=8) is None
    assert bad(percent=0) is None and bad(percent=100) is None and bad(threshold=-3.5) is None
    assert bad(max_gap=n) is None and bad(min_width=n) is None
    assert bad(bin0=97, nbins=4000, span=8) == "bin0" and bad(bin0=n + 1, nbins=8, span=8) == "bin0"
    assert bad(bin0=0xFFFFFFF8, nbins=16, span=8) == "bin0"
    assert bad(nbins=7, span=7) == "nbins" and bad(nbins=0) == "nbins"
    assert bad(span=7) == "span" and bad(span=0) == "span" and bad(span=24) == "span" and bad(nbins=16, span=32) == "span"
    assert bad(percent=101) == "percent"
    for t in (np.nan, np.inf, -np.inf):
        assert bad(threshold=t) == "threshold"
    assert bad(max_gap=n + 1) == "max_gap"
    assert bad(min_width=0) == "min_width" and bad(min_width=n + 1) == "min_width"


PLAN_RULES = [(8, {}), (256, {}), (4096, {}), (4096, dict(span=8)), (65536, {}), (65536, dict(span=65536)), (1 << 20, {}),
              (1 << 20, dict(span=8)), (1 << 20, dict(span=1 << 20)), (1 << 20, dict(bin0=5, nbins=1000, span=8))]
PLAN_ROWS = (1, 3, 300, 70_000, 1 << 24)


@pytest.mark.parametrize("case,nrows", list(itertools.product(range(len(PLAN_RULES)), PLAN_ROWS)))
def test_the_plan_of_a_call(plan, case, nrows):
    """every (row, span) gets a workgroup and every row one; chunks of rows cover every row once and in order; the floors of
    a chunk stay within the cap; LDS stays within what a workgroup may have, and holds the keys of a span that is said to
    sit there"""
    n, fields = PLAN_RULES[case]
    rule = dn.rule_of(n, **fields)
    k, p = _constants(plan), _plan(plan, rule, nrows)
    assert p["nspans"] == rule["nbins"] // rule["span"]
    assert p["chunk_rows"] >= 1 and p["chunk_rows"] * p["nspans"] * 4 <= k["floor_bytes"]
    assert p["floor_bytes"] == min(nrows, p["chunk_rows"]) * p["nspans"] * 4 <= k["floor_bytes"] <= 64 << 20
    assert p["keys_in_lds"] == (rule["span"] <= k["lds_keys"])
    assert p["lds_floor"] >= 4 * (256 + 3 + (rule["span"] if p["keys_in_lds"] else 0))
    assert p["lds_floor"] <= k["lds_max"] and p["lds_segments"] <= k["lds_max"]
    assert k["tile"] % k["threads"] == 0
    most = 200_000
    if -(-nrows // p["chunk_rows"]) > most:
        nrows = p["chunk_rows"] * (most - 1) + 1            # (as many chunks as the test walks, the last one short)
    rows = (SIZE * (4 * most))()
    count = plan.detect_chunks(C.byref(capi.DetectRule(**rule)), nrows, most, rows)
    assert count <= most
    r0, nr, gfloor, gseg = np.array(rows[: 4 * count], dtype=np.int64).reshape(count, 4).T
    assert r0[0] == 0 and np.all(r0[1:] == (r0 + nr)[:-1]) and r0[-1] + nr[-1] == nrows
    assert np.all(nr >= 1) and np.all(nr <= p["chunk_rows"]) and np.all(nr[:-1] == p["chunk_rows"])
    assert np.all(gfloor == nr * p["nspans"]) and np.all(gseg == nr) and gfloor.max() < 2 ** 31


def test_no_rows_no_chunks(plan):
    rows = (SIZE * 4)()
    assert plan.detect_chunks(C.byref(capi.DetectRule(**dn.rule_of(512))), 0, 1, rows) == 0


# ---- the two statements of the rule --------------------------------------------------------------------------------------------

def test_keys_order_the_floats():
    x = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], np.float32)
    k = dn.key(x).astype(np.int64)
    assert np.all(np.diff(k) > 0)
    assert np.array_equal(dn.unkey(dn.key(x)).view(np.uint32), x.view(np.uint32))
    nans = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0xFFFFFFFF], np.uint32).view(np.float32)
    assert np.all((dn.key(nans) > k[-1]) | (dn.key(nans) < k[0]))


@pytest.mark.parametrize("block", range(10))
def test_the_restatement_equals_the_second_opinion(block):
    """300 random cases: n from 8 to 4096, windows, spans, percents 0 ... 100, thresholds of both signs, rows with NaN, +-inf
    and +-0, constant rows"""
    sizes = (8, 16, 24, 64, 100, 256, 1000, 1024, 4096)
    segments = 0
    for i in range(30):
        seed = 30 * block + i
        n = sizes[seed % len(sizes)]
        rows, rule = dn.random_case(seed, n, 2 if n > 1000 else 4)
        a, b = dn.detect(rows, rule), dn.detect_loop(rows, rule)
        assert dn.same(a, b), (seed, n, rule)
        segments += int(a[1].sum())
    print("detect-reference: block %d: %d kept segments in 30 cases" % (block, segments))
    assert segments > 0


def test_known_answers():
    n = 64
    const = np.full((1, n), -37.25, np.float32)
    rule = dn.rule_of(n, bin0=8, nbins=48, span=16, threshold=0.0)
    for f in (dn.detect, dn.detect_loop):
        recs, counts, floors = f(const, rule)
        # a constant row with threshold 0: one segment over the whole window
        assert counts.tolist() == [1] and np.all(floors == np.float32(-37.25))
        assert recs[0].tolist() == [(8, 55, 8, 48, -37.25, -37.25)]
        # ... with a threshold above 0: none
        recs, counts, _ = f(const, dict(rule, threshold=0.5))
        assert counts.tolist() == [0] and recs[0].size == 0
        # percent 0 and 100: the span's minimum and maximum, NaNs left out, -0 below +0
        x = np.random.default_rng(5).normal(size=(1, n)).astype(np.float32)
        x[0, 9], x[0, 30], x[0, 31] = np.nan, -0.0, 0.0
        w = x[0, 8:56].reshape(3, 16)
        lo = f(x, dict(rule, percent=0))[2]
        hi = f(x, dict(rule, percent=100))[2]
        assert np.array_equal(lo[0], np.nanmin(w, axis=1)) and np.array_equal(hi[0], np.nanmax(w, axis=1))
        z = np.array([[0.0, -0.0] * 4], np.float32)
        assert np.signbit(f(z, dn.rule_of(8, percent=0))[2][0, 0]) and not np.signbit(f(z, dn.rule_of(8, percent=100))[2][0, 0])
        # an all-NaN span: a NaN floor (0x7FC00000) and no detection in it, whatever the threshold
        x = np.zeros((1, n), np.float32)
        x[0, 24:40] = np.nan
        x[0, 50] = 20.0
        recs, counts, floors = f(x, dict(rule, threshold=-1.0))
        assert floors.view(np.uint32)[0].tolist() == [dn.key(np.float32(0.0)) ^ 0x80000000, dn.NAN_BITS, 0]
        assert [tuple(r)[:4] for r in recs[0]] == [(8, 23, 8, 16), (40, 55, 50, 16)]
        # segments: a gap of max_gap is bridged, one more is not; min_width drops the narrow one; the peak is the first of equals
        x = np.zeros((1, n), np.float32)
        x[0, [10, 12, 15, 16, 40]] = [5.0, 7.0, 7.0, 6.0, 9.0]
        recs, counts, _ = f(x, dn.rule_of(n, span=64, threshold=1.0, max_gap=1))
        assert [tuple(r)[:4] for r in recs[0]] == [(10, 12, 12, 2), (15, 16, 15, 2), (40, 40, 40, 1)]
        recs, counts, _ = f(x, dn.rule_of(n, span=64, threshold=1.0, max_gap=2, min_width=2))
        assert [tuple(r) for r in recs[0]] == [(10, 16, 12, 4, 7.0, 0.0)] and counts.tolist() == [1]


# ---- the end-to-end inputs on the reference alone --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted(dn.PLANTED))
def test_planted_streams_keep_their_margin_on_the_reference(n):
    """The GPU test demands the integer fields of the device's records to equal those of the restatement on the REFERENCE's
    row.  That can hold only if no bin of the reference's row lies near its threshold: none nearer than 1 dB, which is
    50 x DB_ATOL, the bound the device's rows are held to.  And the mask of the spectrum tests leaves out next to nothing."""
    _, _, F, mean = dn.planted(n)
    rule = dn.rule_of(n)
    row = mean.astype(np.float32)[None]
    recs, counts, floors = dn.detect(row, rule)
    t = np.repeat(floors[0].astype(np.float64) + rule["threshold"], rule["span"])
    nearest = float(np.abs(mean - t).min())
    out = int((mean < mean.max() - sa.MASK_DB).sum())
    print("detect-reference: planted n=%d F=%d: %d segments, nearest bin %.2f dB from its threshold, %d bins outside the mask"
          % (n, F, int(counts[0]), nearest, out))
    assert nearest >= 1.0 and 1.0 >= 50 * DB_ATOL * 0.999
    assert out <= MASK_OUT_SHARE * n
    # every carrier lies in a segment, every segment's peak is a carrier, the lone carriers have segments of their own
    bins = dn.planted_bins(n)
    assert set(int(r["peak_bin"]) for r in recs[0]) <= set(bins)
    assert all(any(r["first"] <= b <= r["last"] for r in recs[0]) for b in bins)
    assert counts[0] == 5
