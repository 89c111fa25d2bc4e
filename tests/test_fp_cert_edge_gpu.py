"""The edge rule graded by the known end diagonals on the device (fp_cert.hip.h, DESIGN.md 4.22, "The edge rule on the known end
diagonals"): with the certificate on and off the results are the oracle's, bit for bit, and the kernel's counters -- 9: the N-free rule,
11: the older rule on reads with N, 14: the graded test only, 10: offered -- equal the counts of the three host entries on the same pairs."""
import functools

import numpy as np
import pytest

import oracle
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu

HCT = align.HumanChimpTwoScoreMatrix
GO, GE = -600, -150
NS = (63, 64, 65, 128, 129, 150, 152, 153, 160)  # lane chunks of 1, 2 and 3 rows; 64 and 128 fill every lane


def make_pair(rng, k, quiet=False):
    """a read in a byte window of 400 .. 1 200 columns.  quiet: one mismatch at most (D < O: no corner is ever tested).  Otherwise two or
    three mismatches on the rows beside a lane-chunk border within 45 rows of one end, an N now and then, the read's first / last bases
    on the window's first / last columns, and one pair in five with the chain head copy + piece copy that the graded test has to refuse"""
    n = NS[k % len(NS)]
    chunk = (n + 63) // 64
    m = int(rng.integers(400, 1201))
    win = rng.integers(0, 4, size=m).astype(np.uint8)
    locus = int(rng.integers(50, m - n - 49))
    read = win[locus:locus + n].copy()
    if quiet:
        if k % 2:
            q = int(rng.integers(0, n))
            read[q] = int(read[q]) ^ 2
        return read, win
    tail = (k // len(NS)) % 2 == 1
    at = lambda q: n - 1 - q if tail else q
    if k % 5 == 2:
        h, L = int(rng.integers(1, 16)), 15
        for q in h + rng.choice(L, size=2, replace=False):
            read[at(int(q))] ^= 2
        d1 = int(rng.integers(2, (m - n - locus if tail else locus) - h - L + 1))
        if not tail:
            win[:h], win[h] = read[:h], (int(read[h]) + 1) % 4
            win[d1 + h:d1 + h + L] = read[h:h + L]
        else:
            win[m - h:], win[m - h - 1] = read[n - h:], (int(read[n - h - 1]) + 1) % 4
            win[m - d1 - h - L:m - d1 - h] = read[n - h - L:n - h]
        return read, win
    for _ in range(2 + (k % 3 == 0)):
        q = int(rng.integers(1, 45 // chunk)) * chunk - int(rng.integers(0, 2))  # the last row of a lane's chunk or the first of the next
        read[at(q)] = int(read[at(q)]) ^ 2 if rng.random() < 0.8 else (int(read[at(q)]) + 1) % 4
    if k % 4 == 0:
        q = int(rng.integers(0, n))
        read[q] = 4
        if k % 8 == 0:
            win[locus + q] = 4
    for side in (0, 1):
        if rng.random() < 0.5:
            L = 1 + int(30 * rng.random() ** 2)
            piece = (read[:L] if side == 0 else read[n - L:]).copy()
            if rng.random() < 0.5:
                piece[int(rng.integers(0, L))] = int(rng.integers(0, 4))
            if side == 0:
                win[:L] = piece
            else:
                win[m - L:] = piece
    return read, win


@functools.lru_cache(maxsize=None)
def batch(seed, count, quiet=False):
    """(reads, windows, oracle result): computed once, shared, not to be changed"""
    rng = np.random.default_rng(seed)
    pairs = [make_pair(rng, k, quiet) for k in range(count)]
    reads, wins = [np.ascontiguousarray(p[0]) for p in pairs], [p[1] for p in pairs]
    return reads, wins, oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=8)


def host_counts(monkeypatch, params, reads, wins):
    """(9, 11, 14) as the three host entries count them, K = 16 like the kernel"""
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")
    old = n_rule = graded = 0
    for a, b in zip(reads, wins):
        o, r, g = (_lib.debug_gapless_certificate(params, a, b, K=16), _lib.debug_gapless_certificate_n(params, a, b, K=16),
                   _lib.debug_gapless_certificate_edge(params, a, b, K=16))
        assert g[0] == (r[0] or g[6]) and (not r[0] or g[:6] == r)
        old += o[0]
        n_rule += 1 if (r[0] and r[5] >= 1) else 0
        graded += g[6]
    return old, n_rule, graded


def run_both(gpu_lib, monkeypatch, call, exp, what):
    """`call` with the certificate on (GNX_FP_CERT=2: whatever the batch size) and off: both the oracle's result, so equal to each other;
    returns counters (9, 11, 14, 10) of the run with it on"""
    from common import assert_same
    counts = None
    monkeypatch.setenv("GNX_FASTPATH", "2")
    for sw in ("2", "0"):
        monkeypatch.setenv("GNX_FP_CERT", sw)
        for which in (9, 10, 11, 14):
            gpu_lib.debug_counter(which)
        got = call()
        assert gpu_lib.get_timing()["fast_path"] == 1
        assert_same(got, exp, "%s (GNX_FP_CERT=%s)" % (what, sw))
        c = tuple(gpu_lib.debug_counter(which) for which in (9, 11, 14, 10))
        if sw == "2":
            counts = c
        else:
            assert c == (0, 0, 0, 0), c
    return counts


def test_batch_with_graded_exits(gpu_lib, monkeypatch):
    """256 pairs, every read length, mismatches beside the lane-chunk borders: the graded test admits some, refuses the chains"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(6100, 256)
    got = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "graded exits")
    want = host_counts(monkeypatch, p, reads, wins)
    print("counters 9 / 11 / 14 / 10:", got, "host entries:", want)
    assert got == want + (256,), (got, want)
    assert got[2] >= 10 and 256 - sum(got[:3]) >= 40  # not vacuous: the graded test admits pairs, and pairs still go through the sweep


def test_batch_without_graded_exits(gpu_lib, monkeypatch):
    """reads with one mismatch at most: D < O, no corner is tested, counter 14 stays 0"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(6200, 128, True)
    got = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "no graded exits")
    want = host_counts(monkeypatch, p, reads, wins)
    assert got == want + (128,), (got, want)
    assert got[2] == 0 and got[0] >= 60


def test_packed_reference(gpu_lib, monkeypatch):
    """the same pairs against the packed resident reference (gnx_align_batch_by_offset): the reference is the windows one after another,
    so that every window keeps its own first and last columns; windows whose 64-base blocks hold an N stay refused"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(6300, 192)
    ref = np.concatenate(wins)
    lens = np.asarray([len(w) for w in wins], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    a_cat = np.concatenate(reads)
    a_off = np.zeros(len(reads) + 1, dtype=np.int64)
    a_off[1:] = np.cumsum([len(r) for r in reads])
    gpu_lib.set_reference(ref)
    got = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch_by_offset(p, a_cat, a_off, starts, lens), exp, "packed reference")
    clean = [not np.any(ref[(s >> 6) << 6:(((s + l - 1) >> 6) + 1) << 6] >= 4) for s, l in zip(starts, lens)]
    want = host_counts(monkeypatch, p, [r for r, c in zip(reads, clean) if c], [w for w, c in zip(wins, clean) if c])
    assert got == want + (192,), (got, want)
    assert got[2] >= 5
