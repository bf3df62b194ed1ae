"""-m gpu: wr_spectrum_rows_detect -- the noise floor of every span and the occupied segments of spectrum rows.

Every test uploads rows made on the host (or makes them on the device with the library's own calls), calls the library and
compares BIT FOR BIT with tests/detect_np.py's restatement on the same rows: the counts, every record's six words, the
floors.  Record arrays are pre-filled with a sentinel, and the entries behind min(count, max_det) must still hold it.
tests/test_detect_reference.py holds the restatement to a second opinion and shows why the end-to-end inputs may be
compared, in their integer fields, with the restatement on the REFERENCE's row."""
import ctypes as C

import numpy as np
import pytest

import detect_np as dn
import specavg_np as sa
from flat_spectrum import flat
from speccases import DB_ATOL
from webradio_amd import capi, synth
from webradio_amd.device import DETECTION, Spectrum, Tuner

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _run(dev, spec, rows, rule, max_det=16, floors=True, rows_dev=None, nrows=None):
    """the call on `rows` (uploaded unless rows_dev is given): (det (nrows, max_det) DETECTION, counts, floors or None)"""
    R = rows.shape[0] if rows_dev is None else nrows
    nspans = rule["nbins"] // rule["span"]
    p = dev.upload(rows) if rows_dev is None else rows_dev
    det_p = dev.upload(np.full(R * max_det * DETECTION.itemsize, SENTINEL, np.uint8)) if max_det else None
    count_p = dev.upload(np.full(R * 4, SENTINEL, np.uint8))
    floor_p = dev.upload(np.full(R * nspans * 4, SENTINEL, np.uint8)) if floors else None
    spec.rows_detect(p, R, capi.DetectRule(**rule), max_det, det_p, count_p, floor_p)
    dev.sync()
    det = dev.download(det_p, R * max_det, DETECTION).reshape(R, max_det) if max_det else np.zeros((R, 0), DETECTION)
    counts = dev.download(count_p, R, np.uint32)
    fl = dev.download(floor_p, R * nspans).reshape(R, nspans) if floors else None
    for q in (det_p, count_p, floor_p) + ((p,) if rows_dev is None else ()):
        if q is not None:
            dev.free(q)
    return det, counts, fl


def _expected(want, R, max_det):
    recs, counts, _ = want
    exp = np.frombuffer(bytes([SENTINEL]) * (R * max_det * DETECTION.itemsize), DETECTION).reshape(R, max_det).copy()
    for r in np.flatnonzero(counts):
        k = min(int(counts[r]), max_det)
        exp[r, :k] = recs[r][:k]
    return exp


def _same(got, want, max_det, what):
    """counts, records (and the sentinel behind them) and floors, to the bit"""
    det, counts, fl = got
    R = counts.size
    assert np.array_equal(counts, want[1]), (what, "counts", np.flatnonzero(counts != want[1])[:8])
    exp = _expected(want, R, max_det)
    if det.tobytes() != exp.tobytes():
        bad = np.flatnonzero((det.view(np.uint8).reshape(R, -1) != exp.view(np.uint8).reshape(R, -1)).any(axis=1))
        r = int(bad[0])
        raise AssertionError("%s: records of %d rows differ; row %d: got %s want %s" % (what, bad.size, r, det[r][:4], exp[r][:4]))
    if fl is not None:
        same = fl.view(np.uint32) == want[2].view(np.uint32)
        assert same.all(), (what, "floors", np.argwhere(~same)[:8], fl[~same][:4], want[2][~same][:4])


def _check(dev, spec, rows, rule, max_det=16, floors=True, what=""):
    want = dn.detect(rows, rule)
    got = _run(dev, spec, rows, rule, max_det, floors)
    _same(got, want, max_det, what or "n=%d rows=%d %s" % (rows.shape[1], rows.shape[0], rule))
    return got, want


@pytest.fixture(scope="module")
def specs(dev):
    made = {}

    def get(n, real=False):
        if (n, real) not in made:
            made[n, real] = Spectrum(dev, n, real=real)
        return made[n, real]
    yield get
    for s in made.values():
        s.destroy()


# ---- random rows ---------------------------------------------------------------------------------------------------------------

# (n, nrows): below a wave, one wave, one small tile; several tiles and the carry; one row, three, three hundred
RANDOM_SHAPES = [(8, 1), (8, 3), (64, 3), (256, 1), (256, 300), (1024, 3), (4096, 1), (4096, 3)]


@pytest.mark.parametrize("n,nrows", RANDOM_SHAPES, ids=["%d-%d" % s for s in RANDOM_SHAPES])
def test_random_rows(dev, specs, n, nrows):
    """averaged-noise rows with carriers, dB and linear; random windows, spans, percents, thresholds of both signs, max_gap
    0 ... 4, min_width 1 ... 4; NaN, +-inf, +-0 sprinkled in; constant rows.  With and without floor_dev, max_det 3 and 16."""
    segments = cut = 0
    for i in range(8 if nrows < 100 else 4):
        seed = 1000 * n + 10 * nrows + i
        rows, rule = dn.random_case(seed, n, nrows)
        max_det = 3 if i % 2 else 16
        (_, counts, _), _ = _check(dev, specs(n), rows, rule, max_det, floors=i % 3 != 2)
        segments += int(counts.sum())
        cut += int((counts > max_det).sum())
    print("detect: random n=%d rows=%d: %d kept segments, %d rows with more than max_det" % (n, nrows, segments, cut))
    assert segments > 0


def test_one_row_of_300_called_alone_equals_its_records_inside_the_batch(dev, specs):
    n = 256
    rows, rule = dn.random_case(77, n, 300)
    det, counts, fl = _run(dev, specs(n), rows, rule)
    assert counts.sum() > 0
    for r in (0, 137, 299):
        d1, c1, f1 = _run(dev, specs(n), rows[r: r + 1], rule)
        assert c1[0] == counts[r] and d1[0].tobytes() == det[r].tobytes()
        assert np.array_equal(f1.view(np.uint32)[0], fl.view(np.uint32)[r])


def test_more_rows_than_a_grid_dimension(dev, specs):
    """70 000 rows of 8 bins: a workgroup per row and span, rows folded into grid.x"""
    n, R = 8, 70_000
    rng = np.random.default_rng(3)
    rows = dn.noise_rows(rng, R, n, False, frames=4)
    rows[rng.integers(0, R, 2000), rng.integers(0, n, 2000)] = rng.choice(dn.SPRINKLE, 2000)
    (_, counts, _), _ = _check(dev, specs(n), rows, dn.rule_of(n, threshold=2.0, max_gap=0), max_det=2)
    print("detect: 70000 rows of 8: %d kept segments, %d rows with more than 2" % (int(counts.sum()), int((counts > 2).sum())))
    assert counts.sum() > 1000 and (counts > 2).any()


def test_more_floors_than_the_scratch_holds_go_in_chunks_of_rows(dev, specs):
    """300 rows of 4096 bins in spans of 8: 153 600 floors, 131 072 fit: two chunks, with floor_dev and through the scratch"""
    n, R = 4096, 300
    rows = dn.noise_rows(np.random.default_rng(4), R, n, False)
    rule = dn.rule_of(n, span=8, threshold=6.0, percent=25)
    for floors in (True, False):
        (_, counts, _), _ = _check(dev, specs(n), rows, rule, max_det=8, floors=floors)
    assert counts[-1] > 0 and counts[0] > 0


# ---- the select on spans that cannot sit in LDS ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,span,percent", [(65536, 1024, 50), (65536, 65536, 50), (65536, 65536, 93), (1 << 20, 1 << 20, 10)],
                         ids=["65536-1024", "65536-65536", "65536-65536-p93", "1048576-1048576"])
def test_large_rows(dev, specs, n, span, percent):
    rng = np.random.default_rng(n + span)
    rows = dn.noise_rows(rng, 1, n, False)
    where = rng.integers(0, n, 64)
    rows[0, where] = rng.choice(dn.SPRINKLE, where.size)
    rows[0, 5000:5003] = -12.0
    rows[0, n - 2:] = -9.0
    (_, counts, fl), _ = _check(dev, specs(n), rows, dn.rule_of(n, span=span, percent=percent, threshold=12.0), max_det=64)
    print("detect: n=%d span=%d: %d kept segments, floor[0] %.3f dB" % (n, span, int(counts[0]), float(fl[0, 0])))
    assert counts[0] >= 2


# ---- edges, at n = 4096 ----------------------------------------------------------------------------------------------------------

N_EDGE = 4096
LOW, HIGH = np.float32(-40.0), np.float32(0.0)


def test_a_merge_and_a_split_across_every_wave_and_tile_border(dev, specs):
    """for every multiple b of 64, g in {max_gap, max_gap + 1} and every offset -(g + 3) ... +2: two hot bins at p = b + offset
    and p + g + 1 -- g cold bins between them -- one row per case, all rows in one call"""
    max_gap = 1
    cases = [(b + off, g) for b in range(64, N_EDGE, 64) for g in (max_gap, max_gap + 1) for off in range(-(g + 3), 3)]
    rows = np.full((len(cases), N_EDGE), LOW, np.float32)
    for r, (p, g) in enumerate(cases):
        rows[r, p], rows[r, p + g + 1] = HIGH, np.float32(1.0)
    (det, counts, _), _ = _check(dev, specs(N_EDGE), rows, dn.rule_of(N_EDGE, max_gap=max_gap), max_det=4)
    for r, (p, g) in enumerate(cases):
        assert counts[r] == (1 if g <= max_gap else 2)
        assert (det[r, 0]["first"], det[r, 0]["last"]) == ((p, p + g + 1) if g <= max_gap else (p, p))
        assert det[r, counts[r] - 1]["peak_bin"] == p + g + 1
    print("detect: %d merge and split cases" % len(cases))


def test_window_edges(dev, specs):
    bin0, nbins, span = 100, 3840, 768
    rule = dn.rule_of(N_EDGE, bin0=bin0, nbins=nbins, span=span, max_gap=1)
    end = bin0 + nbins
    plant = [[end - 3, end - 2, end - 1],           # a segment ending on the window's last bin
             [bin0, bin0 + 1],                      # one starting on its first bin
             [bin0 - 1], [end],                     # a hot bin just outside, on either side: nothing
             [bin0 - 1, bin0, end - 1, end],        # ... and touching hot bins inside: segments of one bin, not two
             [bin0, end - 1],                       # segments do not wrap round the window's ends
             []]                                    # none hot
    rows = np.full((len(plant), N_EDGE), LOW, np.float32)
    for r, bins in enumerate(plant):
        rows[r, bins] = HIGH
    (det, counts, _), _ = _check(dev, specs(N_EDGE), rows, rule, max_det=4)
    assert counts.tolist() == [1, 1, 0, 0, 2, 2, 0]
    assert (det[0, 0]["first"], det[0, 0]["last"]) == (end - 3, end - 1)
    assert (det[1, 0]["first"], det[1, 0]["last"]) == (bin0, bin0 + 1)
    assert [(d["first"], d["last"]) for d in det[4, :2]] == [(bin0, bin0), (end - 1, end - 1)]
    # all bins hot: a threshold below the floor; whole row and window
    noise = dn.noise_rows(np.random.default_rng(6), 2, N_EDGE, False)
    for r in (rule, dn.rule_of(N_EDGE)):
        (det, counts, _), _ = _check(dev, specs(N_EDGE), noise, dict(r, threshold=-30.0, percent=0), max_det=4)
        assert counts.tolist() == [1, 1] and det[0, 0]["hot"] == r["nbins"] and det[0, 0]["first"] == r["bin0"]


def test_min_width_and_max_det(dev, specs):
    """segments of 1 and 3 bins in turn, 10 bins apart, across three tiles: min_width = 2 drops every second one, so the
    output index is not the segment index; more kept segments than max_det; max_det = 0 only counts"""
    rows = np.full((2, N_EDGE), LOW, np.float32)
    starts = np.arange(5, N_EDGE - 10, 10)
    for i, s in enumerate(starts):
        rows[0, s: s + (3 if i % 2 else 1)] = HIGH + np.float32(i % 7)
    rows[1, 2000:2003] = HIGH
    spec = specs(N_EDGE)
    rule = dn.rule_of(N_EDGE, max_gap=0, min_width=2)
    kept = len(starts) // 2
    for max_det in (kept + 5, 7, 1):
        (det, counts, _), _ = _check(dev, spec, rows, rule, max_det=max_det)
        assert counts.tolist() == [kept, 1]
        assert det[0, 0]["first"] == starts[1] and det[0, 0]["hot"] == 3
    (det, counts, _), _ = _check(dev, spec, rows, rule, max_det=0)
    assert counts.tolist() == [kept, 1] and det.size == 0
    (_, counts, _), _ = _check(dev, spec, rows, dict(rule, min_width=1), max_det=len(starts))
    assert counts.tolist() == [len(starts), 1]


# ---- end to end ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted(dn.PLANTED))
def test_planted_carriers_end_to_end(dev, oracle, n):
    """the planted stream through Spectrum.batch_avg (mean, dB), rows_detect on the row in device memory: the integer fields
    of every record equal those of the restatement on the REFERENCE's row, peak and floor lie within DB_ATOL of the
    reference's, everything is bit-identical to the restatement on the DEVICE's own row, and bin_hz of a record's peak_bin is
    a planted carrier's frequency -- of the lone carriers (the first bin, DC, the last bin) each its own record's."""
    stream, hop, F, ref_mean = dn.planted(n)
    rule = dn.rule_of(n)
    spec = Spectrum(dev, n, hop)
    p = dev.upload(stream)
    row_p = dev.malloc(n * 4)
    spec.batch_avg(p, F, row_p)
    got = _run(dev, spec, None, rule, max_det=16, rows_dev=row_p, nrows=1)
    row = dev.download(row_p, n)[None]
    recs, counts, floors = spec.detect(row_p, 1)                # the convenience call, the default rule
    dev.free(row_p)
    dev.free(p)
    _same(got, dn.detect(row, rule), 16, "planted n=%d, the device's own row" % n)
    assert counts[0] == got[1][0] and recs[0].tobytes() == got[0][0, : counts[0]].tobytes()
    assert np.array_equal(floors.view(np.uint32), got[2].view(np.uint32))
    want = dn.detect(ref_mean.astype(np.float32)[None], rule)
    assert counts[0] == want[1][0] == 5
    d_peak = d_floor = 0.0
    for g, w in zip(recs[0], want[0][0]):
        assert [g[f] for f in ("first", "last", "peak_bin", "hot")] == [w[f] for f in ("first", "last", "peak_bin", "hot")]
        j = (int(w["peak_bin"]) - rule["bin0"]) // rule["span"]
        ref_floor = np.sort(ref_mean[j * rule["span"]: (j + 1) * rule["span"]])[(rule["span"] - 1) * 50 // 100]
        d_peak = max(d_peak, abs(float(g["peak"]) - ref_mean[w["peak_bin"]]))
        d_floor = max(d_floor, abs(float(g["floor"]) - ref_floor))
    print("detect: planted n=%d: peak within %.3g dB, floor within %.3g dB of the reference's (bound %.3g)" % (n, d_peak, d_floor, DB_ATOL))
    assert d_peak <= DB_ATOL and d_floor <= DB_ATOL
    rate, centre = dn.PLANTED_RATE, dn.PLANTED_CENTRE
    freqs = [centre + (b - n // 2) * rate / n for b in dn.planted_bins(n)]
    got_hz = [spec.bin_hz(rate, centre, int(g["peak_bin"])) for g in recs[0]]
    assert all(hz in freqs for hz in got_hz)
    assert got_hz[0] == freqs[0] == centre - rate / 2 and got_hz[2] == centre and got_hz[-1] == freqs[-1]
    assert spec.bin_hz(rate, centre, (int(recs[0][1]["first"]) + int(recs[0][1]["last"])) / 2) == (freqs[1] + freqs[2]) / 2
    spec.destroy()


FS, CHAN_RATE, AUDIO_RATE, D1 = 2_400_000, 240_000, 48_000, 10


def test_channel_spectra_of_a_tuner(dev, oracle):
    """64 receivers, 256-point channel spectra (Tuner.chan_spectra), a carrier off centre in three of them: on the window
    of the channel filter's passband those rows have exactly one detection with the right peak_bin; every row equals the
    restatement on the device's rows.  (One unaveraged frame: the threshold is 25 dB, out of the noise's own reach.)"""
    n, k1, first = 256, 272, 16
    ifs = [(c - 32) * 30_000 + 99 for c in range(64)]
    targets = {5: 10, 30: -7, 55: 25}
    rng = np.random.default_rng(1)
    t = np.arange(k1 * D1)
    z = (rng.normal(size=t.size) + 1j * rng.normal(size=t.size)) * 1e-2
    for c, off in targets.items():
        z += 0.1 * np.exp(2j * np.pi * (ifs[c] + off * CHAN_RATE / n) * t / FS)
    x = dev.upload(np.ascontiguousarray(z.astype(np.complex64)).view(np.float32))
    tun = Tuner(dev, FS, 64, k1 * D1, capi.WR_NCO_ROTATE)
    chans = [tun.add_receiver(f, 100_000, CHAN_RATE, capi.WR_FM, 8_000, AUDIO_RATE) for f in ifs]
    spec = Spectrum(dev, n)
    tun.submit_device(x, k1 * D1)
    rows_p = dev.malloc(64 * n * 4)
    assert tun.chan_spectra(spec, first, db_dev=rows_p) == 64
    rule = dn.rule_of(n, bin0=88, nbins=80, span=80, threshold=25.0)
    got = _run(dev, spec, None, rule, max_det=8, rows_dev=rows_p, nrows=64)
    rows = dev.download(rows_p, 64 * n).reshape(64, n)
    _same(got, dn.detect(rows, rule), 8, "channel spectra")
    for c, off in targets.items():
        slot = tun.slot(chans[c])
        assert got[1][slot] == 1 and got[0][slot, 0]["peak_bin"] == n // 2 + off
        assert spec.bin_hz(CHAN_RATE, ifs[c], int(got[0][slot, 0]["peak_bin"])) == ifs[c] + off * CHAN_RATE / n
    dev.free(rows_p)
    spec.destroy()
    tun.destroy()
    dev.free(x)


def test_a_real_spectrum_with_the_window_on_the_upper_half(dev, oracle, specs):
    """a tone on bin 100 of a 1024-point real spectrum: the whole row shows it twice, mirrored; the upper half once"""
    n, hop, F, k = 1024, 512, 8, 100
    total = sa.span(n, hop, F)
    x = flat(total, seed=12) * np.float32(1.0 / 64) + (0.02 * np.cos(2 * np.pi * k * np.arange(total) / n)).astype(np.float32)
    spec = specs(n, real=True)
    mine = Spectrum(dev, n, hop, real=True)
    p = dev.upload(x)
    row_p = dev.malloc(n * 4)
    mine.batch_avg(p, F, row_p)
    row = None
    for rule, peaks in ((dn.rule_of(n, bin0=n // 2, nbins=n // 2, span=n // 2), [n // 2 + k]),
                        (dn.rule_of(n), [n // 2 - k, n // 2 + k])):
        got = _run(dev, spec, None, rule, max_det=8, rows_dev=row_p, nrows=1)
        row = dev.download(row_p, n)[None] if row is None else row
        _same(got, dn.detect(row, rule), 8, "real spectrum")
        assert got[0][0, : got[1][0]]["peak_bin"].tolist() == peaks
    dev.free(row_p)
    dev.free(p)
    mine.destroy()


def test_beside_an_open_streaming_launch(dev, specs):
    """the call on a device whose tuner has a streaming launch open closes the launch and gives the same records"""
    n, K2 = 512, 1024
    rows, rule = dn.random_case(4242, n, 5)
    spec = specs(n)
    before = _run(dev, spec, rows, rule)
    ifs = [(c - 4) * 30_000 + 99 for c in range(8)]
    x = dev.upload(synth.fm_stream(K2 * 50, FS, ifs[::3], amp=0.1))
    t = Tuner(dev, FS, 8, K2 * 50, capi.WR_NCO_ROTATE)
    for f in ifs:
        t.add_receiver(f, 100_000, CHAN_RATE, capi.WR_FM, 8_000, AUDIO_RATE)
    t.streaming(True)
    p = dev.upload(rows)
    out = [dev.upload(np.zeros(5 * 16 * 24, np.uint8)), dev.upload(np.zeros(5, np.uint32))]
    t.submit_device(x, K2 * 50)
    assert t.stream_info()[0] is True
    spec.rows_detect(p, 5, capi.DetectRule(**rule), 16, out[0], out[1])
    assert t.stream_info()[0] is False
    dev.sync()
    counts = dev.download(out[1], 5, np.uint32)
    det = dev.download(out[0], 5 * 16, DETECTION).reshape(5, 16)
    assert np.array_equal(counts, before[1]) and counts.sum() > 0
    for r in range(5):
        k = min(int(counts[r]), 16)
        assert det[r, :k].tobytes() == before[0][r, :k].tobytes()
    t.destroy()
    for q in out + [p, x]:
        dev.free(q)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------

def test_argument_errors(dev, specs):
    lib, n = dev.lib, 64
    spec = specs(n)
    rows = dev.upload(np.zeros(n, np.float32))
    marker = np.full(16, 7, np.uint32)
    count, det = dev.upload(marker), dev.upload(np.zeros(24, np.uint8))
    vp = C.c_void_p
    good = capi.DetectRule(**dn.rule_of(n))

    def call(s=spec.h, r=rows, nrows=1, rule=good, max_det=1, d=det, c=count):
        return lib.wr_spectrum_rows_detect(s, vp(r) if r else None, nrows, C.byref(rule) if rule else None, max_det,
                                           vp(d) if d else None, vp(c) if c else None, None)

    for bad in (dict(s=None), dict(r=None), dict(rule=None), dict(d=None), dict(c=None)):
        assert call(**bad) == capi.WR_ERR_ARG
        assert b"wr_spectrum_rows_detect" in lib.wr_last_error()
    for field, value in (("bin0", 1), ("nbins", 4), ("span", 24), ("span", 4), ("percent", 101), ("threshold", float("nan")),
                         ("threshold", float("inf")), ("max_gap", n + 1), ("min_width", 0), ("min_width", n + 1)):
        assert call(rule=capi.DetectRule(**dn.rule_of(n, **{field: value}))) == capi.WR_ERR_ARG
        msg = lib.wr_last_error()
        assert b"wr_spectrum_rows_detect" in msg and field.encode() in msg, msg
    # no rows: nothing written, even without rows; max_det = 0 needs no records
    assert call(nrows=0) == capi.WR_OK and call(nrows=0, r=None) == capi.WR_OK
    dev.sync()
    assert np.array_equal(dev.download(count, 16, np.uint32), marker)
    assert call(max_det=0, d=None) == capi.WR_OK
    dev.sync()
    assert dev.download(count, 16, np.uint32).tolist() == [0] + [7] * 15   # (a constant row, threshold 10: nothing is hot)
    for q in (rows, count, det):
        dev.free(q)
