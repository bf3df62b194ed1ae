"""What the tests of wr_spectrum_rows_detect share: two statements of the rule of include/webradio_amd.h (the band scan), the
random rows and rules both are tried on, and the planted streams of the end-to-end tests.  No tests here.

A rule is a dict with the fields of wr_detect_rule (rule_of fills in wr_detect_rule_default's values).

detect()      the vectorised restatement, all rows at once: keys sorted per span, the hot bins by flatnonzero, the starts
              by diff, a segment's peak by maximum.reduceat over key << 32 | ~index.
detect_loop() the second opinion: a plain loop over the bins of a row, one state machine, nothing shared with the first
              but the definition of a key.
Both return (records, counts, floors): a list of DETECTION arrays, one per row, every kept segment of the row; the counts
(uint32); the floors (rows, nbins / span) float32."""
import functools

import numpy as np

import specavg_np as sa
from flat_spectrum import flat

DETECTION = np.dtype([("first", np.uint32), ("last", np.uint32), ("peak_bin", np.uint32), ("hot", np.uint32),
                      ("peak", np.float32), ("floor", np.float32)])
FIELDS = ("bin0", "nbins", "span", "percent", "threshold", "linear", "max_gap", "min_width")
NAN_BITS = 0x7FC00000


def rule_of(n, **fields):
    rule = dict(bin0=0, nbins=n, span=min(n, 1024), percent=50, threshold=10.0, linear=0, max_gap=1, min_width=1)
    assert set(fields) <= set(FIELDS)
    rule.update(fields)
    return rule


def key(x):
    """the order of floats as unsigned integers; NaNs fall outside [key(-inf), key(inf)]"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31 == 1, u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000))


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def threshold_of(floors, rule):
    with np.errstate(all="ignore"):
        t = floors * np.float32(rule["threshold"]) if rule["linear"] else floors + np.float32(rule["threshold"])
    assert t.dtype == np.float32
    return t


# ---- the vectorised restatement --------------------------------------------------------------------------------------------

def floors_of(rows, rule):
    rows = np.atleast_2d(np.asarray(rows, np.float32))
    R = rows.shape[0]
    span, nspans = rule["span"], rule["nbins"] // rule["span"]
    w = rows[:, rule["bin0"]: rule["bin0"] + rule["nbins"]].reshape(R, nspans, span)
    k = key(w).astype(np.uint64)
    nan = w != w
    k[nan] = 1 << 32                                        # behind every key
    k.sort(axis=-1)
    m = (~nan).sum(axis=-1)
    rank = np.where(m > 0, ((m - 1) * rule["percent"]) // 100, 0)
    fk = np.take_along_axis(k, rank[..., None], axis=-1)[..., 0]
    bits = unkey((fk & 0xFFFFFFFF).astype(np.uint32)).view(np.uint32)
    return np.where(m > 0, bits, np.uint32(NAN_BITS)).astype(np.uint32).view(np.float32)


def _split(recs, row_of, R):
    counts = np.bincount(row_of, minlength=R).astype(np.uint32)
    ends = np.cumsum(counts)
    return [recs[e - c: e] for c, e in zip(counts, ends)], counts


def detect(rows, rule):
    rows = np.atleast_2d(np.asarray(rows, np.float32))
    R = rows.shape[0]
    bin0, nbins, span = rule["bin0"], rule["nbins"], rule["span"]
    floors = floors_of(rows, rule)
    w = rows[:, bin0: bin0 + nbins]
    with np.errstate(invalid="ignore"):
        hot = w >= np.repeat(threshold_of(floors, rule), span, axis=-1)
    at = np.flatnonzero(hot.ravel())
    if not at.size:
        return [np.zeros(0, DETECTION) for _ in range(R)], np.zeros(R, np.uint32), floors
    row, b = at // nbins, at % nbins
    start = np.ones(at.size, bool)
    start[1:] = (row[1:] != row[:-1]) | (np.diff(b) - 1 > rule["max_gap"])
    s = np.flatnonzero(start)
    e = np.r_[s[1:], at.size]
    packed = key(w.ravel()[at]).astype(np.uint64) << np.uint64(32) | (~(b + bin0).astype(np.uint32)).astype(np.uint64)
    top = np.maximum.reduceat(packed, s)
    recs = np.zeros(s.size, DETECTION)
    recs["first"], recs["last"], recs["hot"] = b[s] + bin0, b[e - 1] + bin0, e - s
    recs["peak_bin"] = ~(top & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    recs["peak"] = unkey((top >> np.uint64(32)).astype(np.uint32))
    recs["floor"] = floors[row[s], (recs["peak_bin"].astype(np.int64) - bin0) // span]
    keep = recs["last"].astype(np.int64) - recs["first"] + 1 >= rule["min_width"]
    out, counts = _split(recs[keep], row[s][keep], R)
    return out, counts, floors


# ---- the second opinion ------------------------------------------------------------------------------------------------------

def _key1(x):
    u = int(np.float32(x).view(np.uint32))
    return u ^ 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def detect_loop(rows, rule):
    rows = np.atleast_2d(np.asarray(rows, np.float32))
    bin0, nbins, span = rule["bin0"], rule["nbins"], rule["span"]
    thr = np.float32(rule["threshold"])
    out, counts, floors = [], [], []
    for x in rows:
        fl = []
        for j in range(nbins // span):
            vals = sorted((v for v in x[bin0 + j * span: bin0 + (j + 1) * span] if v == v), key=_key1)
            fl.append(vals[((len(vals) - 1) * rule["percent"]) // 100] if vals else np.uint32(NAN_BITS).view(np.float32))
        recs, cur, last = [], None, None

        def close():
            if cur is not None and last - cur["first"] + 1 >= rule["min_width"]:
                recs.append((cur["first"], last, cur["peak_bin"], cur["hot"], x[cur["peak_bin"]],
                             fl[(cur["peak_bin"] - bin0) // span]))

        for k in range(bin0, bin0 + nbins):
            f = fl[(k - bin0) // span]
            with np.errstate(all="ignore"):
                t = f * thr if rule["linear"] else f + thr
            if not x[k] >= t:
                continue
            if cur is None or k - last - 1 > rule["max_gap"]:
                close()
                cur = dict(first=k, hot=0, peak_bin=k)
            cur["hot"] += 1
            if _key1(x[k]) > _key1(x[cur["peak_bin"]]):
                cur["peak_bin"] = k
            last = k
        close()
        out.append(np.array(recs, DETECTION) if recs else np.zeros(0, DETECTION))
        counts.append(len(recs))
        floors.append(np.array(fl, np.float32))
    return out, np.array(counts, np.uint32), np.stack(floors)


def same(a, b):
    """two results agree in every count, every word of every record and every floor"""
    (ra, ca, fa), (rb, cb, fb) = a, b
    return (np.array_equal(ca, cb) and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and len(ra) == len(rb)
            and all(x.tobytes() == y.tobytes() for x, y in zip(ra, rb)))


# ---- random rows and rules ---------------------------------------------------------------------------------------------------

def noise_rows(rng, nrows, n, linear, frames=16):
    """averaged-noise rows (the mean of `frames` exponentials a bin, about -40 dB) with up to six carriers 12 to 40 dB above
    it, some of them a few bins wide: dB, or the powers themselves; float32"""
    p = rng.exponential(1.0, (nrows, frames, n)).mean(axis=1) * 1e-4
    for r in range(nrows):
        for _ in range(int(rng.integers(0, 7))):
            at, width = int(rng.integers(0, n)), int(rng.integers(1, 6))
            p[r, at: at + width] *= 10.0 ** (rng.uniform(12.0, 40.0, len(p[r, at: at + width])) / 10.0)
    return (p if linear else 10.0 * np.log10(p)).astype(np.float32)


SPRINKLE = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)


def random_rule(rng, n, linear):
    nbins = int(rng.integers(8, n + 1))
    if rng.integers(0, 3) == 0:
        nbins = n
    bin0 = int(rng.integers(0, n - nbins + 1))
    spans = [s for s in range(8, nbins + 1) if nbins % s == 0]
    thr = float(rng.uniform(1.5, 30.0)) if linear else float(rng.uniform(-3.0, 15.0))
    if linear and rng.integers(0, 4) == 0:
        thr = -thr
    return rule_of(n, bin0=bin0, nbins=nbins, span=int(rng.choice(spans)), percent=int(rng.choice([0, 100, *rng.integers(0, 101, 6)])),
                   threshold=float(np.float32(thr)), linear=int(linear), max_gap=int(rng.integers(0, 5)), min_width=int(rng.integers(1, 5)))


def random_case(seed, n, nrows):
    """(rows (nrows, n) float32, rule): dB or linear by the seed; one row in three with NaN, +-inf and +-0 sprinkled in (now
    and then a whole stretch of NaN); one row in eight constant"""
    rng = np.random.default_rng(seed)
    linear = bool(seed & 1)
    rows = noise_rows(rng, nrows, n, linear)
    for r in range(nrows):
        if rng.integers(0, 3) == 0:
            where = rng.integers(0, n, max(1, n // 16))
            rows[r, where] = rng.choice(SPRINKLE, where.size)
            if rng.integers(0, 2) == 0:
                a = int(rng.integers(0, n))
                rows[r, a: a + int(rng.integers(1, 40))] = np.nan
        if rng.integers(0, 8) == 0:
            rows[r] = rows[r, 0]
    return rows, random_rule(rng, n, linear)


# ---- the planted streams of the end-to-end tests -----------------------------------------------------------------------------

# n: (carrier amplitude, frames); half-overlapped
PLANTED = {512: (0.02, 16), 4096: (0.02, 16), 65536: (0.005, 9)}
PLANTED_RATE, PLANTED_CENTRE = 2_400_000, 100_000_000.0


def planted_bins(n):
    """shifted-row bins of the carriers: the first and the last bin, DC, a pair two bins apart and a pair three bins apart"""
    return [0, n // 8, n // 8 + 2, n // 2, n // 2 + n // 4, n // 2 + n // 4 + 3, n - 1]


@functools.lru_cache(maxsize=None)
def planted(n):
    """(stream interleaved float32, hop, frames, the reference's mean dB row in float64) of the planted stream of n points"""
    amp, F = PLANTED[n]
    hop = n // 2
    total = sa.span(n, hop, F)
    z = (flat(2 * total, seed=900 + n) * np.float32(1.0 / 64)).view(np.complex64).astype(np.complex128)
    t = np.arange(total)
    for b in planted_bins(n):
        z += amp * np.exp(2j * np.pi * ((b - n // 2) * t % n) / n)
    stream = np.ascontiguousarray(z.astype(np.complex64)).view(np.float32)
    mean = sa.reference_db(sa.group_frames(stream, False, n, hop, F))[0]
    stream.setflags(write=False)
    mean.setflags(write=False)
    return stream, hop, F, mean
