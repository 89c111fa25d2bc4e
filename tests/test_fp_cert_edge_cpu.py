"""The gapless certificate's edge rule graded by the known end diagonals ("The edge rule on the known end diagonals") on
the host, through gnx_debug_gapless_certificate_edge: whatever it certifies must be the oracle's score and CIGAR, bit for bit.  No GPU.

The rule is restated here in python (the old rule with N, then the graded corners).  The pairs are built for it: reads of 63 .. 160 bases
in windows of a few hundred columns, 2 .. 4 mismatches packed into the first or last 45 rows, 0 .. 3 N, copies of the read's first or
last 1 .. 40 bases with 0 .. 2 mismatches on the window's first / last columns (large A0 / Am), copies of 1 .. 15-base pieces beside the
locus and a few diagonals off it; K is the largest value item 5 admits at the planted locus."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bench
import oracle
import test_fp_cert_cpu as base
import test_fp_cert_deficit_cpu as dm
import test_fp_cert_n_cpu as ncpu
from gonomics_amd import _lib, align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCT = align.HumanChimpTwoScoreMatrix
# (most pairs where the rule has a second branch to decide in: under -1000 / -1 lambda is 92 and item 5 admits no K worth scanning with)
COUNTS = {"hct_600_150": 11000, "hct_1000_1": 500, "asym_600_150": 3000, "hct_400_30": 1000, "hct_300_150": 500, "nneg_600_150": 4000, "bad_600_150": 500}
SETTINGS = [s[:4] + (COUNTS[s[0]],) for s in ncpu.SETTINGS]  # the settings of tests/test_fp_cert_n_cpu.py
assert sum(s[4] for s in SETTINGS) >= 20000
MIN_NEW, MIN_NEW_GRADED, MIN_NEW_N = 1000, 200, 200  # admitted by the graded test only / of them with a grade j >= 1 deciding / with N: conditions
# HCT with s(A, C) = -110: with e = -150 an A over C loses 200 = lambda, an A over T 446 (the boundary unit E = O + lambda j)
ONEOFF = [row[:] for row in HCT]
ONEOFF[0][1] = -110


@pytest.fixture(autouse=True)
def _entry(monkeypatch):
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


# ---- the rule restated -----------------------------------------------------------------------------------------------------------------
def restate(mx, o, e, a, b, c, K, known=True):
    """the certificate on diagonal c (item 3 is the caller's): None, or (d*, score, edge, nu, admitted by the graded test only, the largest
    grade at which the bounds without the bytes refuse or -1).  known = False: the graded test with A0 = Am = 0 (the sensitivity run)."""
    w, R, lam = ncpu.rebased_n(mx, e)
    n, m, O = len(a), len(b), -o
    if o >= 0 or lam <= 0 or any(R[x] <= 0 or R[x] <= max(int(w[x][y]) for y in range(5) if y != x) for x in range(4)):
        return None
    if n < 1 or K < 1 or K > n or m < n + 2 or c <= 0 or c >= m - n or np.any(a >= 5) or np.any(b >= 5):
        return None
    ai = a.astype(np.int64)
    mid = w[ai, b[c:c + n].astype(np.int64)]
    loss = np.asarray(R, dtype=np.int64)[ai] - mid
    f, g = w[ai, b[:n].astype(np.int64)] - mid, w[ai, b[m - n:].astype(np.int64)] - mid
    if np.any(np.cumsum(f) > 0):
        return None
    D, nu = int(loss.sum()), int(np.sum(a == 4))
    if D == O or D >= 2 * O:
        return None
    J, J1 = D // lam + nu, (D + O) // lam + nu
    if n - J <= 0 or n - J1 <= 0 or (K - 1) * (3 + J) >= n - J or (K - 1) * (2 + J1) >= n - J1:
        return None
    G = np.cumsum(g[::-1])
    best, ds = (int(G.max()), int(np.nonzero(G == G.max())[0][-1]) + 1) if G.max() >= 0 else (0, 0)
    if ds >= n:
        return None
    score = int(mid.sum()) + best + 2 * o + e * (n + m)
    if D < O:
        return ds, score, False, nu, False, -1
    J3 = (D - O) // lam + nu
    if (K - 1) * (4 + J3) >= n - J3:
        return None
    Ts = lambda j: (1 + j + nu) * (K - 1) + j + nu
    Tt = lambda j: (2 + j + nu) * (K - 1) + j + nu
    T1, T2 = Ts(J3 - nu), Tt(J3 - nu)
    if T1 + T2 >= n:
        return None
    P = np.concatenate([[0], np.cumsum(loss)])

    def E(p, q):
        p = min(p, n)
        return int(P[p] + D - P[n - min(q, n - p)])
    if E(T1, T2) < O and E(T2, T1) < O:
        return ds, score, True, nu, False, -1
    nf0 = np.nonzero((a != 4) & (a != b[:n]))[0]
    nfm = np.nonzero((a != 4) & (a != b[m - n:]))[0][::-1]
    jdec = -1
    for j in range((D - O) // lam + 1):
        A0 = (int(nf0[j]) if j < len(nf0) else n) if known else 0
        Am = (n - 1 - int(nfm[j]) if j < len(nfm) else n) if known else 0
        lim = O + lam * j
        if not (E(min(A0, Ts(j)), min(Ts(j) + Am, Tt(j))) < lim and E(min(Ts(j) + A0, Tt(j)), min(Am, Ts(j))) < lim):
            return None
        if not (E(Ts(j), Tt(j)) < lim and E(Tt(j), Ts(j)) < lim):
            jdec = j
    return ds, score, True, nu, True, jdec


def one_diagonal(a, b, K):
    """item 3 as gnx_cert_scan_naive has it: the diagonal when the exact K-mer matches are non-empty and share one, else None"""
    n, m = len(a), len(b)
    ab, bb = bytes(a), bytes(b & 3)
    table = {}
    for q in range(n - K + 1):
        if 4 not in a[q:q + K]:
            table.setdefault(ab[q:q + K], []).append(q)
    diag = set()
    for j in range(m - K + 1):
        for q in table.get(bb[j:j + K], ()):
            diag.add(j - q)
    return diag.pop() if len(diag) == 1 else None


# ---- the pairs -------------------------------------------------------------------------------------------------------------------------
def make_case(rng, k):
    """one adversarial pair: (read, window, planted locus)"""
    n = [63, 64, 65, 128, 129, 150, 152, 153, 160][k % 9] if k % 4 == 0 else int(rng.integers(63, 161))
    m = n + int(rng.integers(100, 320))
    win = rng.integers(0, 4, size=m).astype(np.uint8)
    locus = int(rng.integers(42, m - n - 41))
    read = win[locus:locus + n].copy()
    if k % 7 == 3:
        # the path the known diagonals are for: the read's first h bases on the window's first columns, the next L rows -- they hold the
        # mismatches -- copied some diagonals off the locus: [h rows] [gap] [L rows] [gap] [the rest on diagonal c] [gap]; or its mirror image
        h, L = int(rng.integers(1, 16)), int(rng.integers(6, 15))
        rows = h + rng.choice(L, size=2, replace=False)
        tail = rng.random() < 0.5
        for q in rows:
            q = n - 1 - int(q) if tail else int(q)
            read[q] = int(read[q]) ^ 2 if rng.random() < 0.7 else (int(read[q]) + int(rng.integers(1, 4))) % 4
        d1 = int(rng.integers(2, (m - n - locus if tail else locus) - h - L + 1))
        if not tail:
            win[:h], win[h] = read[:h], (int(read[h]) + 1) % 4
            win[d1 + h:d1 + h + L] = read[h:h + L]
        else:
            win[m - h:], win[m - h - 1] = read[n - h:], (int(read[n - h - 1]) + 1) % 4
            win[m - d1 - h - L:m - d1 - h] = read[n - h - L:n - h]
        return read, win, locus
    end = int(rng.integers(0, 3))  # the mismatches: in the first 45 rows, in the last 45, in either
    for _ in range(int(rng.choice([2, 2, 3, 3, 3, 4]))):
        q = int(rng.integers(0, 45))
        q = q if end == 0 or (end == 2 and rng.random() < 0.5) else n - 1 - q
        read[q] = int(read[q]) ^ 2 if rng.random() < 0.7 else (int(read[q]) + int(rng.integers(1, 4))) % 4  # (transitions lose least: three fit under two gap opens)
    for _ in range(int(rng.choice([0, 0, 0, 1, 1, 2, 3]))):  # N over a window N or over whatever the window has
        q = int(rng.integers(0, n))
        read[q] = 4
        if rng.random() < 0.4:
            win[locus + q] = 4
    for side in (0, 1):  # a copy of the read's first / last 1 .. 40 bases on the window's first / last columns, 0 .. 2 mismatches in it
        if rng.random() < 0.45:
            L = 1 + int(40 * rng.random() ** 2)
            piece = (read[:L] if side == 0 else read[n - L:]).copy()
            for _ in range(int(rng.integers(0, 3))):
                piece[int(rng.integers(0, L))] = int(rng.integers(0, 4))
            if side == 0:
                win[:L] = piece
            else:
                win[m - L:] = piece
    for _ in range(int(rng.choice([0, 1, 2, 2]))):  # copies of 1 .. 15-base pieces beside the locus and one to three diagonals off it
        L = int(rng.integers(1, 16))
        q = int(rng.integers(0, 46 - L)) if rng.random() < 0.5 else n - L - int(rng.integers(0, 46 - L))
        s = int(rng.integers(1, 4)) * (1 if rng.random() < 0.5 else -1)
        col = [locus - L - int(rng.integers(0, 4)), locus + n + int(rng.integers(0, 4)), locus + q + s, int(rng.integers(0, m - L + 1))][int(rng.integers(0, 4))]
        col = min(max(col, 0), m - L)
        piece = read[q:q + L]
        win[col:col + L] = np.where(piece == 4, win[col:col + L], piece)
    return read, win, locus


@functools.lru_cache(maxsize=None)
def cases(count):
    rng = np.random.default_rng(52077 + count)
    return [make_case(rng, k) for k in range(count)]


@functools.lru_cache(maxsize=None)
def run_setting(name):
    """(cases, K per case, the entry's result per case, oracle result): once per setting"""
    _, mx, go, ge, count = [s for s in SETTINGS if s[0] == name][0]
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    cs = cases(count)
    Ks = [ncpu.k_max_n(mx, go, ge, a, b, locus) for a, b, locus in cs]
    got = [_lib.debug_gapless_certificate_edge(p, a, b, K=K) for (a, b, _), K in zip(cs, Ks)]
    exp = oracle.align_batch(oracle.MODE_AFFINE, mx, go, ge, [c[0] for c in cs], [c[1] for c in cs], threads=8)
    return cs, Ks, got, exp


def oracle_runs(exp, k):
    scores, ops, off = exp
    return int(scores[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])]


@pytest.mark.parametrize("name", [s[0] for s in SETTINGS])
def test_certified_equals_oracle_and_restatement(name):
    cs, Ks, got, exp = run_setting(name)
    _, mx, go, ge, _ = [s for s in SETTINGS if s[0] == name][0]
    certified = [(k,) + g[1:4] for k, g in enumerate(got) if g[0]]
    print("%s: %d of %d certified, %d by the graded test only" % (name, len(certified), len(cs), sum(1 for g in got if g[6])))
    base.check_against_oracle(cs, certified, exp)
    for k, g in enumerate(got):
        a, b, locus = cs[k]
        if g[0]:
            assert restate(mx, go, ge, a, b, g[1], Ks[k]) == g[2:], (k, g)
        elif restate(mx, go, ge, a, b, locus, Ks[k]) is not None:  # the restatement certifies at the planted locus: item 3 must be what refused
            assert one_diagonal(a, b, Ks[k]) != locus, (k, g)
    if name == "bad_600_150":
        assert not certified


def test_the_graded_test_is_exercised():
    """not vacuous: pairs only the graded test admits, of them with a grade j >= 1 at which the bounds without the bytes refuse, with N"""
    new = graded = with_n = 0
    for s in SETTINGS:
        got = run_setting(s[0])[2]
        new += sum(1 for g in got if g[6])
        graded += sum(1 for g in got if g[6] and g[7] >= 1)
        with_n += sum(1 for g in got if g[6] and g[5] >= 1)
    print("admitted by the graded test only: %d, a grade j >= 1 deciding: %d, with N: %d" % (new, graded, with_n))
    assert new >= MIN_NEW and graded >= MIN_NEW_GRADED and with_n >= MIN_NEW_N, (new, graded, with_n)


def test_without_the_known_diagonals_the_cases_go_wrong():
    """sensitivity: the same cases through the restatement with A0 = Am = 0 -- the corners E(0, Ts) and E(Ts, 0) -- certify pairs whose
    closed form is not the oracle's result, so the generator sees the bounds' absence"""
    wrong = seen = 0
    for name, mx, go, ge, _ in SETTINGS:
        cs, Ks, got, exp = run_setting(name)
        for k, (a, b, locus) in enumerate(cs):
            if got[k][0]:
                continue
            r = restate(mx, go, ge, a, b, locus, Ks[k], known=False)
            if r is None or one_diagonal(a, b, Ks[k]) != locus:
                continue
            seen += 1
            score, runs = oracle_runs(exp, k)
            wrong += not (r[1] == score and base.closed_form(len(a), len(b), locus, r[0]) == runs)
    print("certified without the bounds and refused with them: %d, wrong: %d" % (seen, wrong))
    assert wrong >= 1


def test_the_older_entry_decides_the_same_where_it_certifies():
    """every pair gnx_debug_gapless_certificate_n certifies is certified identically by the new entry, and not counted as new"""
    seen = 0
    for name, mx, go, ge, _ in SETTINGS:
        cs, Ks, got, _ = run_setting(name)
        p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
        for k, (a, b, _) in enumerate(cs):
            old = _lib.debug_gapless_certificate_n(p, a, b, K=Ks[k])
            assert old[0] == (got[k][0] and not got[k][6]), (name, k, old, got[k])
            if old[0]:
                assert got[k][:6] == old and got[k][7] == -1
                seen += 1
    assert seen >= 1000


# ---- boundary units --------------------------------------------------------------------------------------------------------------------
def one(mx, go, ge, a, b, K=16):
    """(the new entry's result, oracle's score, oracle's runs); a certified pair is checked against the oracle here"""
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    res = _lib.debug_gapless_certificate_edge(p, a, b, K=K)
    score, route = oracle.align_one(oracle.MODE_AFFINE, mx, go, ge, a, b)
    if res[0]:
        assert res[3] == score and base.closed_form(len(a), len(b), res[1], res[2]) == route, (res, score, route)
    return res, score, route


def differ(x):
    return (int(x) + 1) % 4


# HCT, gapOpen -600, K = 16, two A-against-T mismatches (D = 892, J3 = 0): Ts(0) = 15, Tt(0) = 30; the old corners hold rows 0 .. 29
@pytest.mark.parametrize("head,accepted", [(15, False), (14, True)])
def test_head_copy_that_reaches_the_second_mismatch(head, accepted):
    """mismatches on rows 20 and 29, the read's first `head` bases on the window's first columns (A0 = head) and an exact copy of rows 15 .. 29
    forty diagonals off the locus.  head = 15: [15 rows on diagonal 0] [gap] [15 rows on the copy] [gap] [the rest on diagonal c] [gap] saves
    892 for one more gap open of 600 and wins -- 15 + A0 = 30 rows hold both mismatches, refused.  head = 14: the corner is rows 0 .. 28 and
    holds one mismatch, accepted by the graded test only (the old corner stays at 30 rows), and the oracle agrees"""
    read, win = dm.pair()
    dm.plant(read, win, 100, (20, 29), 0, 3)
    win[:head] = read[:head]
    win[head] = differ(read[head])
    win[55:70] = read[15:30]
    win[54], win[70] = differ(read[14]), differ(read[30])
    res, score, route = one(HCT, -600, -150, read, win)
    assert not _lib.debug_gapless_certificate_n(_lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150), read, win, K=16)[0]
    if accepted:
        assert res[0] and res[1] == 100 and res[6] and res[7] == 0
    else:
        assert not res[0]
        assert route == [(15, 0), (40, 1), (15, 0), (60, 1), (120, 0), (150, 1)], route


@pytest.mark.parametrize("tail,accepted", [(15, False), (14, True)])
def test_tail_copy_that_reaches_the_second_mismatch(tail, accepted):
    """the mirror image: mismatches on rows 120 and 129, the read's last `tail` bases on the window's last columns (Am = tail), rows 120 .. 134
    copied forty diagonals past the locus"""
    read, win = dm.pair()
    dm.plant(read, win, 100, (120, 129), 0, 3)
    win[400 - tail:] = read[150 - tail:]
    win[399 - tail] = differ(read[149 - tail])
    win[260:275] = read[120:135]
    win[259], win[275] = differ(read[119]), differ(read[135])
    res, score, route = one(HCT, -600, -150, read, win)
    assert not _lib.debug_gapless_certificate_n(_lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150), read, win, K=16)[0]
    if accepted:
        assert res[0] and res[1] == 100 and res[2] == tail and res[6] and res[7] == 0
    else:
        assert not res[0]
        assert route == [(100, 1), (120, 0), (40, 1), (15, 0), (110, 1), (15, 0)], route


@pytest.mark.parametrize("go,accepted", [(-692, False), (-693, True)])
def test_a_corner_that_equals_the_graded_limit(go, accepted):
    """the one-off matrix (lambda = 200), K = 15: A over T on rows 10 and 33 (2 x 446), A over C on row 75 (200), D = 1092.  Row 0 is
    non-free on diagonal 0, rows 1 .. 4 are free, row 5 is not: A0(0) = 0, A0(1) = 5.  Grade 0 holds rows 0 .. 13 (446), grade 1 rows
    0 .. 33: E = 892 = O + lambda with O = 692, refused; O = 693 accepts at 892 = O + lambda - 1"""
    read, win = dm.pair()
    dm.plant(read, win, 100, (10, 33), 0, 3)
    dm.plant(read, win, 100, (75,), 0, 1)
    win[0] = differ(read[0])
    win[1:5] = read[1:5]
    win[5] = differ(read[5])
    assert ncpu.rebased_n(ONEOFF, -150)[2] == 200 and ncpu.deficit_n(ONEOFF, -150, read, win, 100) == 1092
    # the reason, not only the outcome: A0(0) = 0 and A0(1) = 5 from the bytes, Ts(1) + A0(1) = 29 + 5 = 34 rows, and their loss is 892
    nf0 = [i for i in range(150) if read[i] != win[i]]
    assert nf0[:2] == [0, 5] and (1 + 1) * 14 + 1 + nf0[1] == 34
    assert ncpu.deficit_n(ONEOFF, -150, read[:14], win, 100) == 446 and ncpu.deficit_n(ONEOFF, -150, read[:34], win, 100) == 892 == 692 + 200 * 1
    res = one(ONEOFF, go, -150, read, win, K=15)[0]
    assert res[0] == accepted
    if accepted:
        assert res[6]
    assert (restate(ONEOFF, go, -150, read, win, 100, 15) is not None) == accepted


def test_deficit_at_one_and_two_gap_opens_stays_refused():
    """two A-against-G mismatches near the head (652): D = O and D = 2 O are refused by the bounds before any corner; one off either is decided"""
    read, win = dm.pair()
    dm.plant(read, win, 100, (3, 8), 0, 2)
    assert ncpu.deficit_n(HCT, -150, read, win, 100) == 652
    assert not one(HCT, -652, -150, read, win)[0][0]
    assert not one(HCT, -326, -150, read, win)[0][0]
    assert one(HCT, -653, -150, read, win)[0][0]  # (D < O: the first branch)
    res = one(HCT, -651, -150, read, win)[0]  # (D = O + 1: rows 3 and 8 lie in the old corner; row 0 .. 2 of a random window are not all free)
    assert res[0] == (restate(HCT, -651, -150, read, win, 100, 16) is not None)


def test_entry_is_a_test_hook(monkeypatch):
    monkeypatch.delenv("GNX_DEBUG_ENTRY")
    read, win = dm.pair()
    with pytest.raises(_lib.GnxError):
        _lib.debug_gapless_certificate_edge(_lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150), read, win)


def test_share_on_the_benchmark_workload():
    """the first 4 000 pairs of the headline workload against its 10 kb chunk, K = 16 like the kernel: what the older entry certifies is
    certified as before, 187 pairs on top by the graded test only (51 of them hold an N; the python restatement gives the same), and every
    one of those equals the oracle"""
    reads, chunk = bench.make_workload(2, 100000)
    reads = reads[:4000]
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150)
    got = [(k,) + tuple(_lib.debug_gapless_certificate_edge(p, reads[k], chunk, K=16)) for k in range(len(reads))]
    new = [g for g in got if g[7]]
    old = sum(1 for g in got if g[1] and not g[7])
    print("certified %d of %d by the older rules, %d by the graded test only (%d of them with N)" % (old, len(reads), len(new), sum(1 for g in new if g[6])))
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, -600, -150, [reads[g[0]] for g in new], [chunk] * len(new), threads=8)
    for x, g in enumerate(new):
        score, want = oracle_runs(exp, x)
        assert g[4] == score and base.closed_form(150, len(chunk), g[2], g[3]) == want, (g, score, want)
        assert restate(HCT, -600, -150, reads[g[0]], chunk, g[2], 16) == g[3:]
    assert old == 2113 + 434
    assert (len(new), sum(1 for g in new if g[6])) == (187, 51)
