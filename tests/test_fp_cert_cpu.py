"""The fast path's gapless certificate on the host, through gnx_debug_gapless_certificate: whatever it certifies must be
the oracle's score and CIGAR, bit for bit.  No GPU: the entry runs a naive K-mer scan and the decision arithmetic the kernel shares.

The property runs on adversarial small pairs (reads of 18 .. 44 bases, windows of up to ~130) with K = the largest value the
"K is long enough" rule admits at the planted locus, so that the rule is exercised at sizes where second copies are common."""
import functools

import numpy as np
import pytest

import asym
import oracle
from gonomics_amd import _lib, align

HCT = align.HumanChimpTwoScoreMatrix
# a matrix that violates item 2: A against C scores like A against A
BAD = [row[:] for row in HCT]
BAD[0][1] = BAD[0][0]

SETTINGS = [("hct_600_150", HCT, -600, -150, 6000), ("hct_400_30", HCT, -400, -30, 3000), ("hct_300_150", HCT, -300, -150, 3000),
            ("hct_1000_1", HCT, -1000, -1, 3000), ("asym_600_150", asym.ASYM, -600, -150, 3000), ("bad_600_150", BAD, -600, -150, 3000)]
assert sum(s[4] for s in SETTINGS) >= 20000


@pytest.fixture(autouse=True)
def _entry(monkeypatch):
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


def k_max(mx, o, e, a, b, c):
    """the largest K item 5 admits for the read on diagonal c (a python restatement of the rule); 1 when the rule admits none"""
    n = len(a)
    if c < 0 or c + n > len(b) or np.any(a >= 4):
        return 6
    w = np.asarray(mx, dtype=np.int64) - 2 * e
    R = [int(w[x][x]) for x in range(4)]
    lam = min(min(R[x] - max(int(w[x][y]) for y in range(5) if y != x), R[x]) for x in range(4))
    if lam <= 0:
        return 6
    deficit = sum(R[int(x)] - int(w[int(x)][int(y)]) for x, y in zip(a, b[c:c + n]))
    J, J1 = deficit // lam, (deficit - o) // lam
    if n - J <= 0 or n - J1 <= 0:
        return 1
    return max(1, min(-((J - n) // (3 + J)), -((J1 - n) // (2 + J1))))


def make_case(rng, k):
    """one adversarial pair: (read, window, planted locus)"""
    sz = 2 if k % 5 == 0 else 4
    n = int(rng.integers(18, 45))
    m = n + int(rng.choice([1, 2, 3, 6, 10, 20, 40, 60, 86, 86]))
    win = rng.integers(0, sz, size=m).astype(np.uint8)
    locus = int(rng.choice([0, 1, m - n - 1, m - n] + [int(x) for x in rng.integers(0, m - n + 1, size=4)]))
    locus = min(max(locus, 0), m - n)
    if k % 4 == 1:  # periodic around the locus
        unit = rng.integers(0, sz, size=int(rng.integers(1, 7))).astype(np.uint8)
        lo, hi = max(0, locus - 2 * len(unit)), min(m, locus + n + 2 * len(unit))
        win[lo:hi] = np.resize(unit, hi - lo)
    read = win[locus:locus + n].copy()
    for _ in range(int(rng.choice([0, 0, 0, 0, 1, 1, 2, 3]))):
        q = int(rng.integers(0, n))
        read[q] = (int(read[q]) + int(rng.integers(1, sz))) % sz
    for _ in range(int(rng.choice([0, 0, 1, 1, 2]))):  # copies and 90 % copies of read pieces
        L = int(rng.integers(1, n + 1))
        q = int(rng.integers(0, n - L + 1))
        piece = read[q:q + L].copy()
        if rng.random() < 0.5:
            piece[rng.random(L) < 0.1] = int(rng.integers(0, sz))
        where = int(rng.integers(0, 5))
        col = [0, m - L, q, m - n + q, int(rng.integers(0, m - L + 1))][where]  # column 0, the window's end, the same rows, anywhere
        win[col:col + L] = piece
    if rng.random() < 0.12:
        win[int(rng.integers(0, m))] = 4
    if rng.random() < 0.05:
        read[int(rng.integers(0, n))] = 4
    return read, win, locus


@functools.lru_cache(maxsize=None)
def cases(count):
    rng = np.random.default_rng(90210 + count)
    return [make_case(rng, k) for k in range(count)]


def closed_form(n, m, c, d):
    runs = [(c, 1), (n - d, 0), (m - n - c, 1)]
    if d > 0:
        runs.append((d, 0))
    return runs


def run_setting(mx, go, ge, count):
    """(certified results [(index, c, d, score)], oracle result) of the first `count` cases"""
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    cs = cases(count)
    certified = []
    for k, (a, b, locus) in enumerate(cs):
        ok, c, d, score = _lib.debug_gapless_certificate(p, a, b, K=k_max(mx, go, ge, a, b, locus))
        if ok:
            certified.append((k, c, d, score))
    exp = oracle.align_batch(oracle.MODE_AFFINE, mx, go, ge, [c[0] for c in cs], [c[1] for c in cs], threads=8)
    return cs, certified, exp


def check_against_oracle(cs, certified, exp):
    scores, ops, off = exp
    for k, c, d, score in certified:
        a, b, _ = cs[k]
        got = closed_form(len(a), len(b), c, d)
        want = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])]
        assert score == int(scores[k]) and got == want, (k, a.tolist(), b.tolist(), c, d, score, int(scores[k]), got, want)


@pytest.mark.parametrize("name,mx,go,ge,count", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_certified_equals_oracle(name, mx, go, ge, count):
    cs, certified, exp = run_setting(mx, go, ge, count)
    print("%s: %d of %d certified, %d with d* > 0" % (name, len(certified), count, sum(1 for x in certified if x[2] > 0)))
    check_against_oracle(cs, certified, exp)
    if name == "bad_600_150":
        assert not certified  # the matrix violates item 2
    if name == "hct_600_150":  # not vacuous
        assert len(certified) * 10 >= count, len(certified)
        assert any(x[2] > 0 for x in certified)


def _one(mx, go, ge, a, b, K):
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    res = _lib.debug_gapless_certificate(p, a, b, K=K)
    score, route = oracle.align_one(oracle.MODE_AFFINE, mx, go, ge, a, b)
    if res[0]:
        assert res[3] == score and closed_form(len(a), len(b), res[1], res[2]) == route, (res, score, route)
    return res


def _base_pair(seed=5, n=44, m=120, c=31):
    rng = np.random.default_rng(seed)
    win = rng.integers(0, 4, size=m).astype(np.uint8)
    return win[c:c + n].copy(), win


def test_deficit_boundary():
    """one A read base against C in the window: deficit = s(A,A) - s(A,C) = 420.  deficit == -o is refused, deficit == -o - 1 accepted"""
    read, win = _base_pair()
    read[20], win[31 + 20] = 0, 1
    assert HCT[0][0] - HCT[0][1] == 420
    assert not _one(HCT, -420, -150, read, win, 8)[0]
    res = _one(HCT, -421, -150, read, win, 8)
    assert res[0] and res[1] == 31 and res[2] == 0


def test_prefix_tie_goes_to_the_diagonal():
    """the read's first three bases equal the window's first three columns: F_1 = F_2 = F_3 = 0, accepted, and the oracle agrees"""
    read, win = _base_pair()
    win[0:3] = read[0:3]
    win[3] = (int(read[3]) + 1) % 4
    res = _one(HCT, -600, -150, read, win, 10)
    assert res[0] and res[1] == 31 and res[2] == 0


def test_two_maxima_of_g_take_the_larger_d():
    """the read's last two bases equal the window's last two columns (and the third does not): G_0 = G_1 = G_2 = 0 -> d* = 2"""
    read, win = _base_pair()
    win[-2:] = read[-2:]
    win[-3] = (int(read[-3]) + 1) % 4
    res = _one(HCT, -600, -150, read, win, 10)
    assert res[0] and res[1] == 31 and res[2] == 2


def test_entry_is_a_test_hook(monkeypatch):
    monkeypatch.delenv("GNX_DEBUG_ENTRY")
    read, win = _base_pair()
    with pytest.raises(_lib.GnxError):
        _lib.debug_gapless_certificate(_lib.make_params(_lib.GNX_AFFINE_GAP, HCT, -600, -150), read, win)
