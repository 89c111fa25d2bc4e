"""The gapless certificate with reads that hold N on the device (fp_cert.hip.h, DESIGN.md 4.22, "Reads that hold N"): with the switch
on and off the results are the oracle's, bit for bit; the kernel's count of N-rule exits (gnx_debug_counter 11) equals the host entry's
(gnx_debug_gapless_certificate_n) on the same pairs, and counter 9 stays the count of the N-free rule (the old host entry)."""
import functools

import numpy as np
import pytest

import oracle
import test_fp_cert_gpu as base
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu

HCT = align.HumanChimpTwoScoreMatrix
GO, GE = -600, -150
NS = (66, 150, 152, 153, 160)
# each kind with 1 .. 2 N in the read; "indel" and "copy" are the N read with an indel / with a second copy of the read in the window
KINDS = ("exact", "mismatch", "tail", "head", "indel", "copy")
# With K = 16 and lambda = 296 the N-aware item 5 admits an exact read with one N from 83 bases on (J1 + nu = 3: 15 x 5 < n - 3) and with
# two N from 100 on: reads of 66 bases certify only without N, the others with 1 .. 2 N as well.


def locus(read, win):
    """the column of the window where the read fits best (make_pair does not return where it put it)"""
    n = len(read)
    view = np.lib.stride_tricks.sliding_window_view(win, n)
    return int(np.argmin(np.sum(view != read, axis=1)))


@functools.lru_cache(maxsize=None)
def batch(seed, count):
    """(reads, windows, oracle result, [(n, m, kind)]): computed once, shared, not to be changed"""
    rng = np.random.default_rng(seed)
    reads, wins, meta = [], [], []
    for k in range(count):
        n = NS[k % len(NS)]
        m = (n + 2, 300, 2000)[(k // len(NS)) % 3]
        kind = KINDS[(k // 2) % len(KINDS)]
        a, b = base.make_pair(rng, n, m, kind)
        a = a.copy()
        c = locus(a, b) if kind != "indel" else None
        for x in rng.choice(len(a), size=1 + k % 2, replace=False):
            a[int(x)] = 4
            if k % 3 == 0 and c is not None:  # over a window N; otherwise over whatever base the window has there
                b[c + int(x)] = 4
        if k % 7 == 6:  # one pair in seven keeps a read without N
            a = np.where(a == 4, np.uint8(1), a).astype(np.uint8)
        reads.append(np.ascontiguousarray(a)); wins.append(b); meta.append((n, m, kind))
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=8)
    return reads, wins, exp, meta


def host_counts(monkeypatch, params, reads, wins):
    """(pairs the old host entry certifies, pairs with N the N-aware entry certifies), K = 16 like the kernel; on reads without N the
    two entries must agree"""
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")
    old = n_rule = 0
    for a, b in zip(reads, wins):
        o, r = _lib.debug_gapless_certificate(params, a, b, K=16), _lib.debug_gapless_certificate_n(params, a, b, K=16)
        if not np.any(a == 4):
            assert r[:4] == o and r[5] == 0
        else:
            assert not o[0]
        old += o[0]
        n_rule += 1 if (r[0] and r[5] >= 1) else 0
    return old, n_rule


def run_both(gpu_lib, monkeypatch, call, exp, what):
    """`call` with the certificate on (GNX_FP_CERT=2: whatever the batch size) and off: both the oracle's result; returns counters
    (9, 10, 11) of the run with it on"""
    from common import assert_same
    counts = None
    monkeypatch.setenv("GNX_FASTPATH", "2")  # no shape rules: batches of one pair take the fast path too
    for sw in ("2", "0"):
        monkeypatch.setenv("GNX_FP_CERT", sw)
        for which in (9, 10, 11):
            gpu_lib.debug_counter(which)
        got = call()
        assert gpu_lib.get_timing()["fast_path"] == 1
        assert_same(got, exp, "%s (GNX_FP_CERT=%s)" % (what, sw))
        c = tuple(gpu_lib.debug_counter(which) for which in (9, 10, 11))
        if sw == "2":
            counts = c
        else:
            assert c == (0, 0, 0), c
    return counts


@pytest.mark.parametrize("count", [1, 8, 9, 203])
def test_batches_of_reads_with_n(gpu_lib, monkeypatch, count):
    """every kind, every read length, windows of n + 2, 300 and 2 000 columns in one batch"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp, meta = batch(5100 + count, count)
    c9, c10, c11 = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "reads with N, %d" % count)
    old, n_rule = host_counts(monkeypatch, p, reads, wins)
    assert c10 == count and (c9, c11) == (old, n_rule), (c9, c11, old, n_rule)
    if count == 203:  # not vacuous: both rules certify, and reads with N go through the sweep as well
        assert c11 >= 20 and c9 >= 5 and count - c9 - c11 >= 40, (c9, c11)


def test_n_over_n_and_beside_a_mismatch(gpu_lib, monkeypatch):
    """150-base reads in 300-column byte windows: an N over a window N, an N over A/C/G/T, two adjacent N, an N beside a mismatch and the
    most N item 5 admits (5) and one more -- counter 11 is decided by the construction"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    rng = np.random.default_rng(5200)
    reads, wins = [], []
    plans = [((40,), True, None), ((40,), False, None), ((0,), False, None), ((149,), False, None), ((63, 64), False, None), ((70,), False, 71),
             ((127, 128), True, 100), ((20, 45, 70, 95, 120), False, None), ((20, 45, 70, 95, 120, 140), False, None)]
    for rows, over_n, mis in plans:
        win = rng.integers(0, 4, size=300).astype(np.uint8)
        win[0], win[299] = win[100], win[249]  # (an N on the first / last row scores the same on the window's first / last column: item 6 ties)
        read = win[100:250].copy()
        if mis is not None:
            read[mis] = (int(read[mis]) + 1) % 4
        for r in rows:
            read[r] = 4
            if over_n:
                win[100 + r] = 4
        reads.append(read); wins.append(win)
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=4)
    c9, c10, c11 = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "constructed")
    assert (c9, c10) == (0, len(plans)) and c11 == host_counts(monkeypatch, p, reads, wins)[1]
    assert c11 == len(plans) - 1  # (a chance second 16-mer aside: ~1e-4 per pair) all but the read with six N


def test_packed_reference(gpu_lib, monkeypatch):
    """reads with N against the packed resident reference (gnx_align_batch_by_offset): a read N over an ordinary reference base; windows
    whose 64-base blocks hold an exception stay refused"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    rng = np.random.default_rng(5300)
    ref = rng.integers(0, 4, size=12000).astype(np.uint8)
    ref[rng.integers(0, 12000, size=3)] = 4
    count = 64
    starts = rng.integers(0, 12000 - 1000, size=count).astype(np.int64)
    lens = np.asarray([(300, 1000, 777, 162)[k % 4] for k in range(count)], dtype=np.int64)
    reads = []
    for k in range(count):
        n = NS[k % len(NS)]
        c = int(rng.integers(1, lens[k] - n))
        r = ref[starts[k] + c:starts[k] + c + n].copy()
        if k % 3 == 1:
            x = int(rng.integers(0, n))
            r[x] = (int(r[x]) + 1) % 4
        if k % 4 != 3:
            for x in rng.choice(n, size=1 + k % 2, replace=False):
                r[int(x)] = 4
        if k % 9 == 8:
            r = np.concatenate([r[:30], r[32:], r[:2]])
        reads.append(np.ascontiguousarray(r))
    a_cat = np.concatenate(reads)
    a_off = np.zeros(count + 1, dtype=np.int64)
    a_off[1:] = np.cumsum([len(r) for r in reads])
    wins = [ref[s:s + l] for s, l in zip(starts, lens)]
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=8)
    gpu_lib.set_reference(ref)
    c9, c10, c11 = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch_by_offset(p, a_cat, a_off, starts, lens), exp, "packed reference")
    clean = [not np.any(ref[(s >> 6) << 6:(((s + l - 1) >> 6) + 1) << 6] >= 4) for s, l in zip(starts, lens)]
    old, n_rule = host_counts(monkeypatch, p, [r for r, c in zip(reads, clean) if c], [w for w, c in zip(wins, clean) if c])
    assert c10 == count and (c9, c11) == (old, n_rule), (c9, c11, old, n_rule)
    assert c11 >= 5 and c9 >= 3
