"""The DCS bank without a GPU: the ten functions are declared and bound with the same argument counts, the header carries
the rule, wr_dcs_word and wr_dcs_step give the rule's numbers (and the restatement's: tests/dcs_np.py), argument errors name
their limits, the restatement the GPU tests compare bits with agrees with itself across cuts, and the detection conditions
hold for it on audio from the oracle chain."""
import ctypes as C
import re

import numpy as np
import pytest

import capicases
import dcs_np
from webradio_amd import DCS_CODES, capi, dcs_step, dcs_word

NAMES = [("wr_dcs_word", 2), ("wr_dcs_step", 2), ("wr_dcs_create", 7), ("wr_dcs_destroy", 1), ("wr_dcs_reset", 2),
         ("wr_dcs_seek", 2), ("wr_dcs_push_rows", 5), ("wr_tuner_dcs_push", 3), ("wr_dcs_read", 6), ("wr_dcs_info", 5)]
PAIRS = [(0o023, 0o047), (0o025, 0o244), (0o026, 0o464), (0o031, 0o627), (0o054, 0o413), (0o072, 0o245), (0o074, 0o174)]
WORDS = [dcs_np.word(c) for c in DCS_CODES]


@pytest.mark.parametrize("name, nargs", NAMES)
def test_declared_and_bound_with_the_same_arguments(name, nargs):
    capicases.declared_and_bound(name, nargs)


def test_header_says_the_rule():
    text = capicases.header()
    assert re.search(r"#define\s+WR_ABI_VERSION\s+6\b", text)
    assert capi.load().wr_abi_version() == 6
    assert re.search(r"Added to 6 later: wr_dcs_word, wr_dcs_step, wr_dcs_create, wr_dcs_destroy, wr_dcs_reset,\s+"
                     r"wr_dcs_seek, wr_dcs_push_rows, wr_tuner_dcs_push, wr_dcs_read, wr_dcs_info\.", text)
    for words in ("d = code | 0x800", "if (p & 1) p ^= 0xC75;  p >>= 1", "word = (p << 12) | d",
                  "step = (672 * 2^32 + (5 * rate) / 2) / (5 * rate)", "g(n) = floor(n * step / 2^29)",
                  "q    = (int64) rint(min(max(v', -64.0f), 64.0f) * 16777216.0f)", "C[g(n)] += q",
                  "B_b  = sum_{c < 8} C[8 e - 184 - f + 8 b + c]", "w_f  = sum_b 2^b * [2 * B_b > max_b B + min_b B]",
                  "agree[k][0] = max_{f, r} (23 - popcount(w_f ^ rot_r(word_k)))",
                  "agree[k][1] = max_{f, r} popcount(w_f ^ rot_r(word_k))", "agree >= 23 - max_errors",
                  "A row that a push leaves out (nrows < max_rows) is reset", "muting audio by code"):
        assert words in text, words


# ---- code words -----------------------------------------------------------------------------------------------------------------

def _word(code):
    w = C.c_uint(0xDEADBEEF)
    return capi.load().wr_dcs_word(code, C.byref(w)), w.value


def test_words():
    assert [_word(c) for c in (0o023, 0o754, 0o412)] == [(0, 0x763813), (0, 0x20F9EC), (0, 0x79C90A)]
    for code in range(512):
        rc, w = _word(code)
        assert rc == capi.WR_OK and w == dcs_np.word(code) == dcs_word(code), oct(code)
        assert w & 0xFFF == code | 0x800 and bin(w).count("1") in (7, 8, 11, 12, 15, 16), oct(code)
    for a, b in PAIRS:
        assert ~dcs_np.word(a) & 0x7FFFFF in dcs_np.rotations(dcs_np.word(b)), (oct(a), oct(b))
        assert dcs_np.partner(WORDS, DCS_CODES.index(a)) == [DCS_CODES.index(b)]
    lib = capi.load()
    assert _word(512)[0] == capi.WR_ERR_ARG and b"wr_dcs_word" in lib.wr_last_error() and b"511" in lib.wr_last_error()
    assert lib.wr_dcs_word(0o023, None) == capi.WR_ERR_ARG


def test_standard_codes():
    assert len(DCS_CODES) == 104 and list(DCS_CODES) == sorted(set(DCS_CODES))
    assert DCS_CODES[0] == 0o023 and DCS_CODES[-1] == 0o754 and all(isinstance(c, int) for c in DCS_CODES)
    seen = {}
    for code, w in zip(DCS_CODES, WORDS):
        for r in dcs_np.rotations(w):
            assert seen.setdefault(r, code) == code, (oct(code), oct(seen[r]))      # no code is a rotation of another


# ---- the bit clock --------------------------------------------------------------------------------------------------------------

def _step(rate):
    s = C.c_uint(0xDEADBEEF)
    return capi.load().wr_dcs_step(rate, C.byref(s)), s.value


@pytest.mark.parametrize("rate", [2_151, 5_000, 8_000, 48_000, 50_000])
def test_step_is_the_integer_formula(rate):
    want = (672 * 2 ** 32 + (5 * rate) // 2) // (5 * rate)
    assert _step(rate) == (capi.WR_OK, want)
    assert dcs_np.step_of(rate) == want == dcs_step(rate) and 1 << 19 <= want <= 1 << 28
    # 134.4 Hz: step / 2^32 bits per frame
    assert abs(want / 2.0 ** 32 * rate - 134.4) < 134.4 * 2.0 ** -19


@pytest.mark.parametrize("rate", [0, 2_000, 2_000_000])
def test_step_refuses(rate):
    rc, _ = _step(rate)
    assert rc == capi.WR_ERR_ARG and dcs_np.step_of(rate) is None
    msg = capi.load().wr_last_error()
    assert b"wr_dcs_step" in msg and b"2^19 .. 2^28" in msg


# ---- argument errors ------------------------------------------------------------------------------------------------------------

def test_argument_errors_carry_their_messages():
    lib = capi.load()
    h = C.c_void_p()
    a = np.zeros(4, np.float32)
    ok = np.array(WORDS + WORDS[:25], np.uint32)
    step = dcs_np.step_of(5_000)

    def create(max_rows, words, ncodes, step, max_errors):
        return lib.wr_dcs_create(C.byref(h), None, max_rows, capi.ptr(words), ncodes, step, max_errors)

    # (the limits are checked in front of the device: a NULL one gets that far only with everything else in order)
    for args, say in (((0, ok, 104, step, 0), b"0 rows (1 .. 65535)"), ((65536, ok, 104, step, 0), b"65536 rows (1 .. 65535)"),
                      ((4, ok, 0, step, 0), b"0 codes (1 .. 128)"), ((4, ok, 129, step, 0), b"129 codes (1 .. 128)"),
                      ((4, ok, 104, (1 << 19) - 1, 0), b"(2^19 .. 2^28)"), ((4, ok, 104, (1 << 28) + 1, 0), b"(2^19 .. 2^28)"),
                      ((4, ok, 104, step, 4), b"max_errors 4 (0 .. 3)"),
                      ((4, np.array([5, 1 << 23], np.uint32), 2, step, 0), b"code 1: the word 0x800000 is not below 2^23"),
                      ((4, ok, 104, step, 3), b"NULL dev")):
        assert create(*args) == capi.WR_ERR_ARG, say
        assert b"wr_dcs_create" in lib.wr_last_error() and say in lib.wr_last_error(), (say, lib.wr_last_error())
        assert not h.value
    for call, name in ((lambda: lib.wr_dcs_create(None, None, 1, capi.ptr(ok), 1, step, 0), b"wr_dcs_create"),
                       (lambda: lib.wr_dcs_reset(None, -1), b"wr_dcs_reset"),
                       (lambda: lib.wr_dcs_seek(None, 0), b"wr_dcs_seek"),
                       (lambda: lib.wr_dcs_push_rows(None, capi.ptr(a), 4, 1, 4), b"wr_dcs_push_rows"),
                       (lambda: lib.wr_tuner_dcs_push(None, None, None), b"wr_tuner_dcs_push"),
                       (lambda: lib.wr_dcs_read(None, capi.ptr(a), None, None, None, None), b"wr_dcs_read"),
                       (lambda: lib.wr_dcs_info(None, None, None, None, None), b"wr_dcs_info"),
                       (lambda: lib.wr_dcs_step(5_000, None), b"wr_dcs_step")):
        assert call() == capi.WR_ERR_ARG, name
        assert name in lib.wr_last_error(), (name, lib.wr_last_error())
    assert lib.wr_dcs_destroy(None) == capi.WR_OK


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def _rows(rate, n):
    """three rows: a code as sent from a fractional bit, a code inverted, no code"""
    return np.stack([dcs_np.signal_row(dcs_np.word(0o023), rate, n, 1, start=0.37),
                     dcs_np.signal_row(dcs_np.word(0o754), rate, n, 2, start=7.9, inverted=True),
                     dcs_np.signal_row(None, rate, n, 3)])


def test_the_restatement_is_the_rule_as_plain_loops():
    """one row, one evaluation at a time, the header's lines with Python integers"""
    rate, n = 2_151, 1_500
    step = dcs_np.step_of(rate)
    v = _rows(rate, n)[0]
    words = WORDS[:3] + [dcs_np.word(0o047)]
    bank = dcs_np.Bank(1, words, step, 1)
    start = 12_345
    bank.seek(start)
    bank.push(v[None, :])
    chips = {}
    q = dcs_np.quantise(v)
    for k in range(n):
        g = ((start + k) * step) >> 29
        chips[g] = chips.get(g, 0) + int(q[k])
    g_end = ((start + n) * step) >> 29
    agree = [[0, 0] for _ in words]
    run = [[0, 0] for _ in words]
    hits = [[0, 0] for _ in words]
    evals = 0
    for e in range(((start * step) >> 29) // 8 + 1, g_end // 8 + 1):
        agree = [[0, 0] for _ in words]
        for f in range(8):
            B = [sum(chips.get(8 * e - 184 - f + 8 * b + c, 0) for c in range(8)) for b in range(23)]
            w = sum(1 << b for b in range(23) if 2 * B[b] > max(B) + min(B))
            for k, word in enumerate(words):
                for rot in dcs_np.rotations(word):
                    x = bin(w ^ rot).count("1")
                    agree[k] = [max(agree[k][0], 23 - x), max(agree[k][1], x)]
        for k in range(len(words)):
            for pol in (0, 1):
                match = agree[k][pol] >= 23 - 1
                hits[k][pol] += match
                run[k][pol] = run[k][pol] + 1 if match else 0
        evals += 1
    assert evals == int(bank.evals[0]) > 60
    assert agree == bank.agree[0].tolist() and run == bank.run[0].tolist() and hits == bank.hits[0].tolist()
    assert hits[0][0] > 30 and hits[3][1] == hits[0][0]


@pytest.mark.parametrize("rate", [2_151, 5_000])
def test_the_restatement_agrees_with_itself_across_cuts(rate):
    n = 3_000
    step = dcs_np.step_of(rate)
    v = _rows(rate, n)
    whole = dcs_np.Bank(3, WORDS, step)
    whole.push(v)
    assert int(whole.evals[0]) == ((n * step) >> 29) // 8
    assert whole.agree[0, 0, 0] == 23 and whole.run[0, 0, 0] >= 8 and whole.run[1, DCS_CODES.index(0o754), 1] >= 8
    for cuts in ([1] * 40 + [7, 500, 501, 1_400], [2_999], [37] * 81, [1_000, 1, 1, 1, 1_997]):
        bank = dcs_np.Bank(3, WORDS, step)
        pos = 0
        for c in cuts + [n - sum(cuts)]:
            bank.push(v[:, pos: pos + c])
            pos += c
        assert pos == n
        for got, want, name in zip(bank.read(), whole.read(), ("agree", "run", "hits", "evals")):
            assert np.array_equal(got, want), (rate, cuts[:3], name)


def test_the_restatement_resets_and_seeks():
    rate, n = 5_000, 2_000
    step = dcs_np.step_of(rate)
    v = _rows(rate, n)
    bank = dcs_np.Bank(3, WORDS, step)
    bank.push(v[:, :1_200])
    before = [a.copy() for a in bank.read()]
    bank.reset(1)
    assert not bank.agree[1].any() and not bank.run[1].any() and not bank.hits[1].any() and bank.evals[1] == 0
    for a, b in zip(before, bank.read()):
        assert np.array_equal(a[[0, 2]], b[[0, 2]])
    bank.push(v[:2, 1_200:])                                   # row 2 is left out: it reads as reset
    assert bank.evals[2] == 0 and not bank.hits[2].any() and bank.evals[1] == bank.evals[0] - before[3][0]
    # a stream that begins beyond 2^64 / step: the same bits as the same stream from a clock that is a multiple of a word
    far = dcs_np.Bank(3, WORDS, step)
    far.seek(2 ** 40 - 5)
    far.push(v)
    assert (far.N * step) > 2 ** 64 and int(far.evals[0]) in (((n * step) >> 29) // 8, ((n * step) >> 29) // 8 + 1)
    assert far.agree[0, 0, 0] == 23 and far.run[0, 0, 0] >= 8


# ---- the detection conditions on the oracle chain ------------------------------------------------------------------------------

def test_detection_on_the_oracle_chain(oracle):
    """the tuner case of test_gpu_dcs.py through the oracle's receivers: at the end of the stream every coded receiver's own
    code has agree = 23 and run >= 8 in its polarity, no other standard code but the own code's inverse partner has
    run >= 2 on any receiver, and the two uncoded receivers have no code with run >= 2"""
    rx = [oracle.Receiver(dcs_np.FS, f, dcs_np.CHAN_PASSBAND, dcs_np.CHAN_RATE, capi.WR_FM, dcs_np.AUDIO_PASSBAND,
                          dcs_np.AUDIO_RATE) for f in dcs_np.IFS]
    bank = dcs_np.Bank(len(rx), WORDS, dcs_np.step_of(dcs_np.AUDIO_RATE))
    for b in range(dcs_np.NBLOCKS):
        iq = dcs_np.fm_block(b)
        audio = np.stack([x.run(iq)[0] for x in rx])
        assert audio.shape == (len(rx), dcs_np.K2)
        bank.push(audio)
    assert list(bank.evals) == [(dcs_np.NBLOCKS * dcs_np.K2 * bank.step >> 29) // 8] * len(rx)
    own_runs, foreign = dcs_np.detection(bank.agree, bank.run, WORDS, range(len(rx)))
    print("oracle: %d evaluations; own codes' run %s; largest run of any other code %d" % (int(bank.evals[0]), own_runs, foreign))
