"""The gapless certificate with reads that hold N ("Reads that hold N") on the host, through
gnx_debug_gapless_certificate_n: whatever it certifies must be the oracle's score and CIGAR, bit for bit.  No GPU.

The pairs come from the generators of tests/test_fp_cert_cpu.py (reads of 18 .. 44 bases) and tests/test_fp_cert_deficit_cpu.py (40 .. 160
bases, mismatches biased to the ends, copies of read pieces); each read then gets 1 .. 3 N -- over a window N or over A/C/G/T, on the
rows around the first and the last 16-mer, next to a mismatch, inside and beside a copy of a read piece planted here, two adjacent, two
16 apart -- and K is the largest value the N-aware item 5 admits at the planted locus (a python restatement below)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import asym
import bench
import oracle
import test_fp_cert_cpu as base
import test_fp_cert_deficit_cpu as dm
from gonomics_amd import _lib, align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCT = align.HumanChimpTwoScoreMatrix
# a matrix whose N row is negative everywhere after the rebasing with e = -150 (w = s + 300): R_N = 0, a skipped N row loses nothing
NNEG = [row[:] for row in HCT]
NNEG[4] = [-420, -380, -400, -310, -350]
# the existing six settings and the R_N = 0 one; more pairs where the rule certifies at all (one setting's 3 000 pairs run in under a second)
COUNTS = {"hct_600_150": 10000, "asym_600_150": 5000}
SETTINGS = [s[:4] + (COUNTS.get(s[0], s[4]),) for s in base.SETTINGS] + [("nneg_600_150", NNEG, -600, -150, 5000)]
assert sum(s[4] for s in SETTINGS) >= 20000
MIN_WITH_N, MIN_WITH_N_EDGE = 1000, 100  # certified with nu >= 1 over all settings / of them through the edge branch: conditions, not measurements


@pytest.fixture(autouse=True)
def _entry(monkeypatch):
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


# ---- the rule restated -----------------------------------------------------------------------------------------------------------------
def rebased_n(mx, e):
    """(w, R with R[4] = R_N, lambda)"""
    w, R, lam = dm.rebased(mx, e)
    return w, R + [max(0, max(int(w[4][y]) for y in range(5)))], lam


def deficit_n(mx, e, a, b, c):
    w, R, _ = rebased_n(mx, e)
    return sum(R[int(x)] - int(w[int(x)][int(y)]) for x, y in zip(a, b[c:c + len(a)]))


def k_max_n(mx, o, e, a, b, c):
    """the largest K the N-aware item 5 admits for the read on diagonal c; 1 when it admits none"""
    n = len(a)
    if c < 0 or c + n > len(b) or np.any(a >= 5) or np.any(b[c:c + n] >= 5):
        return 6
    _, _, lam = rebased_n(mx, e)
    if lam <= 0:
        return 6
    D, O, nu = deficit_n(mx, e, a, b, c), -o, int(np.sum(a == 4))
    J, J1 = D // lam + nu, (D + O) // lam + nu
    if n - J <= 0 or n - J1 <= 0:
        return 1
    k = min(-((J - n) // (3 + J)), -((J1 - n) // (2 + J1)))
    if O < D < 2 * O:
        J3 = (D - O) // lam + nu
        if n - J3 <= 0:
            return 1
        k = min(k, -((J3 - n) // (4 + J3)))
    return max(1, k)


# ---- the pairs -------------------------------------------------------------------------------------------------------------------------
def add_n(rng, k, read, win, locus):
    """1 .. 3 N into the read of a generated pair (both arrays are changed in place)"""
    n, m = len(read), len(win)
    mode = k % 8
    fixed = [0, 15, 16, n - 17, n - 16, n - 1]
    mism = [i for i in range(n) if read[i] != win[locus + i]]
    if mode == 0:  # the rows around the first and the last 16-mer
        rows = [fixed[int(x)] for x in rng.choice(6, size=int(rng.integers(1, 4)), replace=False)]
    elif mode == 1 and mism:  # next to a mismatch
        q = mism[int(rng.integers(0, len(mism)))]
        rows = [q + (1 if rng.random() < 0.5 else -1)]
    elif mode == 2:  # two adjacent
        q = int(rng.integers(0, n - 1))
        rows = [q, q + 1]
    elif mode == 3:  # two 16 apart
        q = int(rng.integers(0, max(1, n - 16)))
        rows = [q, q + 16]
    elif mode in (4, 5):  # inside (4) / beside (5) a copy of a read piece planted on the window's edges or just off the locus
        L = int(rng.integers(2, min(n, 24) + 1))
        q = [0, n - L, int(rng.integers(0, n - L + 1))][int(rng.integers(0, 3))]
        rows = [q + int(rng.integers(0, L))] if mode == 4 else [q - 1 if rng.random() < 0.5 else q + L]
        before = rng.random() < 0.5  # the copy holds the read's base (N placed afterwards), or the N itself (inside) as a window N
        piece = read[q:q + L].copy()
        if not before and mode == 4:
            piece[rows[0] - q] = 4
        col = [0, m - L, locus + q + int(rng.choice([-3, -2, -1, 1, 2, 3])), int(rng.integers(0, m - L + 1))][int(rng.integers(0, 4))]
        col = min(max(col, 0), m - L)
        win[col:col + L] = piece
    else:  # anywhere
        rows = [int(x) for x in rng.integers(0, n, size=int(rng.integers(1, 4)))]
    for i in rows:
        i = min(max(int(i), 0), n - 1)
        read[i] = 4
        if rng.random() < 0.4:  # over a window N; otherwise over whatever A/C/G/T the window has there
            win[locus + i] = 4
    return read, win, locus


def make_case(rng, k):
    src = base if k % 4 == 3 else dm  # three in four from the long-read generator: the edge branch needs reads that item 5 admits with J3 + nu
    read, win, locus = src.make_case(rng, k)
    if k % 3 == 0:  # one in three keeps one mismatch at most, so that reads with several N still fall under item 5
        mism = [i for i in range(len(read)) if read[i] != win[locus + i]]
        for i in mism[1:] if rng.random() < 0.5 else mism[:-1]:
            read[i] = win[locus + i]
    return add_n(rng, k, read, win, locus)


@functools.lru_cache(maxsize=None)
def cases(count):
    rng = np.random.default_rng(40455 + count)
    return [make_case(rng, k) for k in range(count)]


@functools.lru_cache(maxsize=None)
def run_setting(name):
    """(cases, certified [(index, c, d, score, edge, nu)], oracle result): once per setting"""
    _, mx, go, ge, count = [s for s in SETTINGS if s[0] == name][0]
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    cs = cases(count)
    certified = []
    for k, (a, b, locus) in enumerate(cs):
        res = _lib.debug_gapless_certificate_n(p, a, b, K=k_max_n(mx, go, ge, a, b, locus))
        if res[0]:
            certified.append((k,) + tuple(res[1:]))
    exp = oracle.align_batch(oracle.MODE_AFFINE, mx, go, ge, [c[0] for c in cs], [c[1] for c in cs], threads=8)
    return cs, certified, exp


@pytest.mark.parametrize("name", [s[0] for s in SETTINGS])
def test_certified_equals_oracle(name):
    cs, certified, exp = run_setting(name)
    with_n = [x for x in certified if x[5] >= 1]
    print("%s: %d of %d certified, %d with N, %d of those by the edge rule" % (name, len(certified), len(cs), len(with_n), sum(1 for x in with_n if x[4])))
    base.check_against_oracle(cs, [x[:4] for x in certified], exp)
    for k, c, d, score, edge, nu in certified:  # the entry's own report against the restatement
        a, b, _ = cs[k]
        mx, go, ge = [(s[1], s[2], s[3]) for s in SETTINGS if s[0] == name][0]
        assert nu == int(np.sum(a == 4)) and edge == (deficit_n(mx, ge, a, b, c) > -go)
    if name == "bad_600_150":
        assert not certified  # the matrix violates item 2


def test_reads_with_n_are_certified_by_both_branches():
    """not vacuous: pairs certified with nu >= 1, and of them through the edge branch, over all settings"""
    with_n = edge = 0
    for s in SETTINGS:
        certified = run_setting(s[0])[1]
        with_n += sum(1 for x in certified if x[5] >= 1)
        edge += sum(1 for x in certified if x[5] >= 1 and x[4])
    print("certified with N: %d, through the edge branch: %d" % (with_n, edge))
    assert with_n >= MIN_WITH_N and edge >= MIN_WITH_N_EDGE, (with_n, edge)


def test_reads_without_n_decide_as_before():
    """on N-free reads the N-aware entry is the old one: accept / refuse, c, d*, score (the cases of the two older tests)"""
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150)
    seen = 0
    for a, b, locus in base.cases(3000)[:1500] + dm.cases(3000)[:1500]:
        if np.any(a == 4):
            continue
        K = dm.k_max(HCT, -600, -150, a, b, locus)
        old, new = _lib.debug_gapless_certificate(p, a, b, K=K), _lib.debug_gapless_certificate_n(p, a, b, K=K)
        assert new[:4] == old and new[5] == 0
        seen += old[0]
    assert seen >= 200  # (not vacuous: a fifteenth of the pairs at the least)


# ---- boundary units --------------------------------------------------------------------------------------------------------------------
def one(mx, go, ge, a, b, K=16):
    """the N-aware certificate's result; a certified pair is checked against the oracle here"""
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    res = _lib.debug_gapless_certificate_n(p, a, b, K=K)
    score, route = oracle.align_one(oracle.MODE_AFFINE, mx, go, ge, a, b)
    if res[0]:
        assert res[3] == score and base.closed_form(len(a), len(b), res[1], res[2]) == route, (res, score, route)
    return res


def test_matrix_terms():
    """HumanChimpTwo, e = -150: R_N = 104 (N against C or G), N over N loses 6; the all-negative N row gives R_N = 0"""
    w, R, lam = rebased_n(HCT, -150)
    assert R[4] == 104 and R[4] - int(w[4][4]) == 6 and lam == 296
    assert rebased_n(NNEG, -150)[1][4] == 0 and rebased_n(HCT, -30)[1][4] == 0


def test_deficit_boundaries_with_an_n():
    """two A-against-G mismatches mid-read (2 x 326) and an N over a window N on row 40 (6): D = 658.  D = O + 1 accepted (edge branch),
    D = O refused, D = O - 1 accepted (first branch), D = 2 O refused, D = 2 O - 2 accepted"""
    read, win = dm.pair()
    dm.plant(read, win, 100, (70, 80), 0, 2)
    dm.plant(read, win, 100, (40,), 4, 4)
    assert deficit_n(HCT, -150, read, win, 100) == 658
    res = one(HCT, -657, -150, read, win)
    assert res[0] and res[1] == 100 and res[4] and res[5] == 1
    assert not one(HCT, -658, -150, read, win)[0]
    res = one(HCT, -659, -150, read, win)
    assert res[0] and not res[4]
    assert not one(HCT, -329, -150, read, win)[0]
    assert one(HCT, -330, -150, read, win)[0]


# HCT, gapOpen -600, K = 16, two A-against-T mismatches (D = 892) and an N over C on row 75 (loses nothing): J3 + nu = 1, T1 = 31, T2 = 46
@pytest.mark.parametrize("rows,accepted", [((30, 45), False), ((30, 104), False), ((45, 119), False), ((30, 118), False), ((31, 103), True),
                                           ((31, 104), True), ((45, 118), True), ((46, 118), True), ((46, 119), True)])
def test_edge_rows_with_one_n(rows, accepted):
    """E(31, 46) = rows 0 .. 30 and 104 .. 149, E(46, 31) = rows 0 .. 45 and 119 .. 149: refused when one of them holds both mismatches.
    (Without the N the corners are 15 / 30 rows: (30, 45) would pass.)"""
    read, win = dm.pair()
    dm.plant(read, win, 100, rows, 0, 3)
    dm.plant(read, win, 100, (75,), 4, 1)
    assert deficit_n(HCT, -150, read, win, 100) == 892
    assert one(HCT, -600, -150, read, win)[0] == accepted
    if rows == (30, 45):
        read[75] = 1
        assert dm.one(HCT, -600, -150, read, win)[0][0]


def test_three_run_path_through_a_copy_cut_by_n_wins():
    """what nu is for.  Two A-against-T mismatches (892) on rows 33 and 38, N over C on rows 15 and 31, and a copy of the read's first 45 bases one
    column into the window: the N cut the copy into exact runs of 15, 15 and 13 bases, so the scan sees nothing off diagonal c, and
    [gap] [45 rows on the copy] [gap] [the rest on diagonal c] [gap] saves the 892 for one more gap open of 600 and at most 24 on the N
    rows (a decision without nu in its thresholds certifies this pair, wrongly).  Without nu the corners are 15 / 30 rows and hold no mismatch; with nu = 2 they are 47 / 62 rows and refuse.  The same
    mismatches on rows 70 and 80, outside either corner, are accepted"""
    read, win = dm.pair()
    dm.plant(read, win, 100, (33, 38), 0, 3)
    dm.plant(read, win, 100, (15, 31), 4, 1)  # (N over C loses nothing: D = 892, J3 = 0)
    win[1:46] = np.where(read[:45] == 4, win[100:145], read[:45])
    win[46] = (int(read[45]) + 1) % 4
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150)
    score, route = oracle.align_one(oracle.MODE_AFFINE, HCT, -600, -150, read, win)
    assert not _lib.debug_gapless_certificate_n(p, read, win, K=16)[0]
    assert route != base.closed_form(150, 400, 100, 0) and route[:3] == [(1, 1), (route[1][0], 0), (99, 1)] and 39 <= route[1][0] <= 45, route
    read, win = dm.pair()
    dm.plant(read, win, 100, (70, 80), 0, 3)
    dm.plant(read, win, 100, (15, 31), 4, 1)  # (N over C loses nothing: D = 892, J3 = 0)
    win[1:46] = np.where(read[:45] == 4, win[100:145], read[:45])
    win[46] = (int(read[45]) + 1) % 4
    res = one(HCT, -600, -150, read, win)
    assert res[0] and res[4] and res[5] == 2


@pytest.mark.parametrize("nu,accepted", [(5, True), (6, False)])
def test_most_n_item_5_admits(nu, accepted):
    """n = 150, K = 16, N over C only (D = 0, J1 = 2): 15 (4 + nu) < 148 - nu holds up to nu = 5"""
    read, win = dm.pair()
    dm.plant(read, win, 100, [20, 45, 70, 95, 120, 140][:nu], 4, 1)
    assert deficit_n(HCT, -150, read, win, 100) == 0
    res = one(HCT, -600, -150, read, win)
    assert res[0] == accepted and (not accepted or res[5] == nu)


def test_wave_decision_with_n_stand_alone(tmp_path):
    """tests/cpp/cert_n_test.cpp: a host program with its own main, built with the address and undefined-behaviour sanitizers and run
    directly -- the N-aware pieces on 64 emulated lanes against gnx_certn_decide for every n from 16 to 160, N on the rows at the lane
    chunks' boundaries, both deficit branches; reads without N against the old gnx_cert_decide"""
    exe = str(tmp_path / "cert_n_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "cert_n_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr


def test_entry_is_a_test_hook(monkeypatch):
    monkeypatch.delenv("GNX_DEBUG_ENTRY")
    read, win = dm.pair()
    with pytest.raises(_lib.GnxError):
        _lib.debug_gapless_certificate_n(_lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150), read, win)


def test_share_on_the_benchmark_workload():
    """the first 4 000 pairs of the headline workload against its 10 kb chunk, K = 16 like the kernel: the N-free reads certify exactly as
    through the old entry, about 430 reads that hold an N certify on top (a python restatement of the rule gave 434: 372 by D < O, 62 by
    the edge rule), and every certified pair equals the oracle"""
    reads, chunk = bench.make_workload(2, 100000)
    reads = reads[:4000]
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150)
    got = [(k,) + tuple(_lib.debug_gapless_certificate_n(p, reads[k], chunk, K=16)) for k in range(len(reads))]
    got = [g for g in got if g[1]]
    old = sum(1 for k in range(len(reads)) if _lib.debug_gapless_certificate(p, reads[k], chunk, K=16)[0])
    free = sum(1 for g in got if g[6] == 0)
    with_n = [g for g in got if g[6] >= 1]
    print("certified %d of %d: %d without N (old entry %d), %d with N (%d of them by the edge rule)" %
          (len(got), len(reads), free, old, len(with_n), sum(1 for g in with_n if g[5])))
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, -600, -150, [reads[g[0]] for g in got], [chunk] * len(got), threads=8)
    scores, ops, off = exp
    for x, g in enumerate(got):
        want = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[x]:off[x + 1]], ops["op"][off[x]:off[x + 1]])]
        assert g[4] == int(scores[x]) and base.closed_form(150, len(chunk), g[2], g[3]) == want, (g, int(scores[x]), want)
    assert free == old
    assert (len(with_n), sum(1 for g in with_n if g[5])) == (434, 62)
