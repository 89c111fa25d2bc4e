"""The gapless certificate's second deficit branch (-o < deficit < -2o with the edge rule) on the host, through
gnx_debug_gapless_certificate like tests/test_fp_cert_cpu.py: whatever it certifies must be the oracle's score and CIGAR, bit for bit.

The property runs on reads of 40 .. 160 bases with 1 .. 4 planted mismatches (biased to the read's ends, where the edge rule decides),
short exact copies of read pieces beside the locus, on the window's first and last columns and one to three columns off the locus, with
K = the largest value item 5 admits at the planted locus.  The boundary units are hand-built pairs, each against the oracle."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bench
import oracle
import test_fp_cert_cpu as base
from gonomics_amd import _lib, align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCT = align.HumanChimpTwoScoreMatrix
SETTINGS = base.SETTINGS  # the existing six (matrix, penalty) settings, 21 000 pairs in all
assert sum(s[4] for s in SETTINGS) >= 20000
MIN_SECOND_BRANCH = 300  # pairs certified with deficit > -o over all settings: fewer would make the property vacuous for the new branch


@pytest.fixture(autouse=True)
def _entry(monkeypatch):
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


def rebased(mx, e):
    """(w, R, lambda) of section 4.22"""
    w = np.asarray(mx, dtype=np.int64) - 2 * e
    R = [int(w[x][x]) for x in range(4)]
    lam = min(min(R[x] - max(int(w[x][y]) for y in range(5) if y != x), R[x]) for x in range(4))
    return w, R, lam


def deficit(mx, e, a, b, c):
    w, R, _ = rebased(mx, e)
    return sum(R[int(x)] - int(w[int(x)][int(y)]) for x, y in zip(a, b[c:c + len(a)]))


def k_max(mx, o, e, a, b, c):
    """the largest K item 5 admits for the read on diagonal c -- a python restatement of its two inequalities and, for
    -o < deficit < -2o, of the third; 1 when the rule admits none"""
    n = len(a)
    if c < 0 or c + n > len(b) or np.any(a >= 4) or np.any(b[c:c + n] >= 5):
        return 6
    _, _, lam = rebased(mx, e)
    if lam <= 0:
        return 6
    D, O = deficit(mx, e, a, b, c), -o
    J, J1 = D // lam, (D + O) // lam
    if n - J <= 0 or n - J1 <= 0:
        return 1
    k = min(-((J - n) // (3 + J)), -((J1 - n) // (2 + J1)))
    if O < D < 2 * O:
        J3 = (D - O) // lam
        if n - J3 <= 0:
            return 1
        k = min(k, -((J3 - n) // (4 + J3)))
    return max(1, k)


def make_case(rng, k):
    """one adversarial pair: (read, window, planted locus)"""
    sz = 2 if k % 6 == 0 else 4
    n = int(rng.integers(40, 161))
    m = n + int(rng.choice([2, 3, 6, 10, 24, 40, 80, 150, 240]))
    win = rng.integers(0, sz, size=m).astype(np.uint8)
    locus = int(rng.choice([0, 1, 1, m - n - 1, m - n - 1, m - n] + [int(x) for x in rng.integers(0, m - n + 1, size=6)]))
    locus = min(max(locus, 0), m - n)
    if k % 5 == 1:  # periodic around the locus
        unit = rng.integers(0, sz, size=int(rng.integers(1, 8))).astype(np.uint8)
        lo, hi = max(0, locus - 2 * len(unit)), min(m, locus + n + 2 * len(unit))
        win[lo:hi] = np.resize(unit, hi - lo)
    read = win[locus:locus + n].copy()
    where = int(rng.integers(0, 4))  # the mismatches: anywhere, at the head, at the tail, in the middle
    for _ in range(int(rng.choice([1, 2, 2, 2, 2, 3, 3, 4]))):
        edge = int(rng.integers(0, min(n, 70)))
        q = [int(rng.integers(0, n)), edge, n - 1 - edge, n // 2 + int(rng.integers(-8, 9))][where if rng.random() < 0.8 else 0]
        read[q] = (int(read[q]) + int(rng.integers(1, sz))) % sz
    for _ in range(int(rng.choice([0, 1, 1, 2, 2]))):  # exact (one in four: 90 %) copies of 1 .. 24-base read pieces
        L = int(rng.integers(1, 25))
        q = [0, n - L, int(rng.integers(0, n - L + 1))][int(rng.integers(0, 3))]
        piece = read[q:q + L].copy()
        if rng.random() < 0.25:
            piece[rng.random(L) < 0.1] = int(rng.integers(0, sz))
        s = int(rng.integers(1, 4)) * (1 if rng.random() < 0.5 else -1)
        # the window's first columns, its last ones, one to three columns in, beside the locus on either side, the same rows one to
        # three diagonals off, anywhere
        col = [0, m - L, abs(s), m - L - abs(s), locus - L - int(rng.integers(0, 4)), locus + n + int(rng.integers(0, 4)), locus + q + s,
               int(rng.integers(0, m - L + 1))][int(rng.integers(0, 8))]
        col = min(max(col, 0), m - L)
        win[col:col + L] = piece
    if rng.random() < 0.06:
        win[int(rng.integers(0, m))] = 4
    if rng.random() < 0.03:
        read[int(rng.integers(0, n))] = 4
    return read, win, locus


@functools.lru_cache(maxsize=None)
def cases(count):
    rng = np.random.default_rng(71077 + count)
    return [make_case(rng, k) for k in range(count)]


@functools.lru_cache(maxsize=None)
def run_setting(name):
    """(cases, certified [(index, c, d, score)], oracle result, how many were certified with deficit > -o): once per setting"""
    _, mx, go, ge, count = [s for s in SETTINGS if s[0] == name][0]
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    cs = cases(count)
    certified = []
    for k, (a, b, locus) in enumerate(cs):
        ok, c, d, score = _lib.debug_gapless_certificate(p, a, b, K=k_max(mx, go, ge, a, b, locus))
        if ok:
            certified.append((k, c, d, score))
    exp = oracle.align_batch(oracle.MODE_AFFINE, mx, go, ge, [c[0] for c in cs], [c[1] for c in cs], threads=8)
    above = sum(1 for k, c, d, score in certified if deficit(mx, ge, cs[k][0], cs[k][1], c) > -go)
    return cs, certified, exp, above


@pytest.mark.parametrize("name", [s[0] for s in SETTINGS])
def test_certified_equals_oracle(name):
    cs, certified, exp, above = run_setting(name)
    print("%s: %d of %d certified, %d of them with deficit > -o" % (name, len(certified), len(cs), above))
    base.check_against_oracle(cs, certified, exp)
    if name == "bad_600_150":
        assert not certified  # the matrix violates item 2


def test_the_second_branch_is_exercised():
    """pairs certified with deficit > -o (the deficit restated here) over all settings: the property above is not vacuous for them"""
    above = {s[0]: run_setting(s[0])[3] for s in SETTINGS}
    print(above)
    assert sum(above.values()) >= MIN_SECOND_BRANCH, above


# ---- boundary units -----------------------------------------------------------------------------------------------------------------
def one(mx, go, ge, a, b, K=16):
    """(certificate's result, oracle's score, oracle's runs); a certified pair is checked against the oracle here"""
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    res = _lib.debug_gapless_certificate(p, a, b, K=K)
    score, route = oracle.align_one(oracle.MODE_AFFINE, mx, go, ge, a, b)
    if res[0]:
        assert res[3] == score and base.closed_form(len(a), len(b), res[1], res[2]) == route, (res, score, route)
    return res, score, route


def pair(n=150, m=400, c=100, seed=11):
    rng = np.random.default_rng(seed)
    win = rng.integers(0, 4, size=m).astype(np.uint8)
    return win[c:c + n].copy(), win


def plant(read, win, c, rows, x, y):
    """read base x against window base y at the given rows of diagonal c"""
    for i in rows:
        read[i], win[c + i] = x, y


def test_deficit_just_above_gap_open():
    """two A read bases against G in the middle: deficit = 2 x 326 = 652.  -o = 651 (deficit = -o + 1): the second branch accepts;
    -o = 652 (deficit == -o) stays refused, like tests/test_fp_cert_cpu.py::test_deficit_boundary; -o = 653 is the first branch"""
    read, win = pair()
    plant(read, win, 100, (70, 80), 0, 2)
    assert HCT[0][0] - HCT[0][2] == 326 and deficit(HCT, -150, read, win, 100) == 652
    res = one(HCT, -651, -150, read, win)[0]
    assert res[0] and res[1] == 100 and res[2] == 0
    assert not one(HCT, -652, -150, read, win)[0][0]
    assert one(HCT, -653, -150, read, win)[0][0]


def test_deficit_just_below_two_gap_opens():
    """deficit 652 again: -o = 326 (deficit == -2o) refused; -o = 327 (deficit = -2o - 2: all losses of this matrix are even)
    accepted.  The odd boundary on the asymmetric matrix: A against C and A against G lose 205 + 122 = 327 = 2 x 164 - 1, accepted;
    A against G and A against T lose 336 = 2 x 168, refused"""
    import asym
    read, win = pair()
    plant(read, win, 100, (70, 80), 0, 2)
    assert not one(HCT, -326, -150, read, win)[0][0]
    assert one(HCT, -327, -150, read, win)[0][0]
    read, win = pair(seed=12)
    plant(read, win, 100, (70,), 0, 1)
    plant(read, win, 100, (80,), 0, 2)
    assert deficit(asym.ASYM, -150, read, win, 100) == 327
    res = one(asym.ASYM, -164, -150, read, win)[0]
    assert res[0] and res[1] == 100
    read, win = pair(seed=12)
    plant(read, win, 100, (70,), 0, 2)
    plant(read, win, 100, (80,), 0, 3)
    assert deficit(asym.ASYM, -150, read, win, 100) == 336
    assert not one(asym.ASYM, -168, -150, read, win)[0][0]  # deficit == -2o
    assert one(asym.ASYM, -169, -150, read, win)[0][0]


# HCT, gapOpen -600, K = 16, deficit 892: J3 = 0, T1 = 15, T2 = 30
@pytest.mark.parametrize("col", [0, 1, 2, 5])
def test_three_run_path_through_a_head_copy_wins(col):
    """two A-against-T mismatches (deficit 892) at rows 3 and 8 and an exact copy of the read's first 12 bases near the window's start:
    [gap] [12 rows on the copy] [gap] [the rest on diagonal c] [gap] saves the 892 for one more gap open of 600.  On the window's very
    first columns (col = 0) that path has two gap runs and item 6 refuses it; one column further in it has three, and only the edge
    rule stands between the pair and a wrong CIGAR"""
    read, win = pair()
    plant(read, win, 100, (3, 8), 0, 3)
    win[col:col + 12] = read[:12]
    win[col + 12] = (int(read[12]) + 1) % 4
    res, score, route = one(HCT, -600, -150, read, win)
    assert not res[0]
    assert route != base.closed_form(150, 400, 100, 0)
    # (the path may leave the copy anywhere after row 8: rows 9 .. 11 match on both diagonals)
    head = route[1 if col else 0][0]
    assert 9 <= head <= 12 and route == ([(col, 1)] if col else []) + [(head, 0), (100 - col, 1), (150 - head, 0), (150, 1)], route


@pytest.mark.parametrize("rows", [(31, 36), (113, 118), (31, 118)])
def test_mismatches_past_the_edge_rows_are_accepted(rows):
    """the same two mismatches at rows T2 + 1 and beyond from either end, the rows around them copied to the window's start (fewer
    than K bases): no three-run path reaches the deficit, accepted, and the oracle agrees"""
    read, win = pair()
    plant(read, win, 100, rows, 0, 3)
    win[1:13] = read[rows[0] - 3:rows[0] + 9]
    res = one(HCT, -600, -150, read, win)[0]
    assert res[0] and res[1] == 100 and res[2] == 0


@pytest.mark.parametrize("rows", [(3, 29), (14, 29), (120, 146), (120, 135), (14, 134), (15, 135), (14, 120), (3, 120)])
def test_mismatches_on_the_edge_rows_are_refused(rows):
    """E(15, 30) (rows 0 .. 14 and 120 .. 149) or E(30, 15) (rows 0 .. 29 and 135 .. 149) holds both mismatches: refused"""
    read, win = pair()
    plant(read, win, 100, rows, 0, 3)
    assert not one(HCT, -600, -150, read, win)[0][0]


@pytest.mark.parametrize("rows", [(20, 130), (3, 30), (119, 135), (15, 119), (30, 134), (14, 119), (30, 135)])
def test_one_mismatch_in_each_corner_is_accepted(rows):
    """neither corner of the edge rule holds both mismatches, 446 < 600: accepted, and the oracle agrees"""
    read, win = pair()
    plant(read, win, 100, rows, 0, 3)
    assert one(HCT, -600, -150, read, win)[0][0]


def test_the_edge_rows_scale_with_k():
    """n = 80, mismatches at rows 38 and 42: K = 16 fails item 5 (J1 = 4: ceil(76 / 6) = 13 < 16); K = 13 passes it and the corners
    are T1 + T2 = 12 + 24 rows, accepted.  Mismatches at rows 11 and 60: K = 13 puts row 60 among the last 24 rows and refuses,
    K = 12 (T1 = 11, T2 = 22: rows 0 .. 10 and 58 .. 79, or rows 0 .. 21 and 69 .. 79) holds one of them at a time and accepts"""
    read, win = pair(n=80, m=300, c=100)
    plant(read, win, 100, (38, 42), 0, 2)
    assert not one(HCT, -600, -150, read, win, K=16)[0][0]
    assert one(HCT, -600, -150, read, win, K=13)[0][0]
    read, win = pair(n=80, m=300, c=100)
    plant(read, win, 100, (11, 60), 0, 2)
    assert not one(HCT, -600, -150, read, win, K=13)[0][0]
    assert one(HCT, -600, -150, read, win, K=12)[0][0]


@pytest.mark.parametrize("n,certifiable", [(94, False), (95, True)])
def test_item_5_with_two_mismatches(n, certifiable):
    """K = 16, gapOpen -600, two mid-read mismatches (deficit 652: J = 2, J1 = 4, J3 = 0): 16 <= ceil((n - 4) / 6) from 95 bases on"""
    hits = 0
    for seed in range(8):
        read, win = pair(n=n, m=300, c=100, seed=40 + seed)
        plant(read, win, 100, (n // 2 - 3, n // 2 + 4), 0, 2)
        hits += one(HCT, -600, -150, read, win)[0][0]
    assert hits == (8 if certifiable else 0)


def test_decision_arithmetic_stand_alone(tmp_path):
    """tests/cpp/cert_decide_test.cpp: fp_cert_decide.h alone in a host program with its own main, built with the address and
    undefined-behaviour sanitizers -- every K from 1 to beyond n on buffers of exactly n and m bytes, each decision against a
    restatement with the losses in an array"""
    exe = str(tmp_path / "cert_decide_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "cert_decide_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr


def test_share_on_the_benchmark_workload():
    """the first 2 000 pairs of the headline workload against its 10 kb chunk, K = 16 like the kernel: the counts of the two branches
    (recorded: DESIGN.md 4.22, profiles/gapless_exit_deficit.json), every certified pair equal to the oracle"""
    reads, chunk = bench.make_workload(2, 100000)
    reads = reads[:2000]
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150)
    got = [(k,) + tuple(_lib.debug_gapless_certificate(p, reads[k], chunk, K=16)) for k in range(len(reads))]
    got = [g for g in got if g[1]]
    first = sum(1 for k, ok, c, d, s in got if deficit(HCT, -150, reads[k], chunk, c) < 600)
    print("certified %d of %d: %d with deficit < -o, %d above" % (len(got), len(reads), first, len(got) - first))
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, -600, -150, [reads[g[0]] for g in got], [chunk] * len(got), threads=8)
    scores, ops, off = exp
    for x, (k, ok, c, d, s) in enumerate(got):
        want = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[x]:off[x + 1]], ops["op"][off[x]:off[x + 1]])]
        assert s == int(scores[x]) and base.closed_form(150, len(chunk), c, d) == want, (k, c, d, s, int(scores[x]), want)
    assert (first, len(got) - first) == (838, 223)
