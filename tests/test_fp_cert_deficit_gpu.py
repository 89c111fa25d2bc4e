"""The gapless certificate's second deficit branch on the device (-o < deficit < -2o with the edge rule): with the
switch on and off the results are the oracle's, bit for bit, and the kernel certifies exactly the pairs the host certificate does."""
import functools

import numpy as np
import pytest

import oracle
import test_fp_cert_gpu as base

pytestmark = pytest.mark.gpu

HCT, GO, GE = base.HCT, base.GO, base.GE
N_CHOICES = (94, 95, 150, 152, 153, 160)  # 94 / 95: item 5's boundary with two mismatches; 152 / 153: the sweep's 19 / 20 rows per lane
KINDS = ("mid2", "end2", "each_end", "three_ag", "end_copy", "indel")


def m_choices(n):
    return (n + 2, 300, 2000)


def mismatch(read, win, c, rows, x=None, y=None):
    """read base x against window base y on diagonal c (by default: the read's base changed to another one)"""
    for i in rows:
        if x is None:
            read[i] = (int(read[i]) + 1 + i % 3) % 4
        else:
            read[i], win[c + i] = x, y


def make_pair(rng, n, m, kind):
    win = rng.integers(0, 4, size=m).astype(np.uint8)
    c = int(rng.integers(1, m - n))
    read = win[c:c + n].copy()
    mid = [int(x) for x in rng.choice(np.arange(n // 2 - 14, n // 2 + 14), size=3, replace=False)]
    if kind == "mid2":
        mismatch(read, win, c, mid[:2])
    elif kind == "end2":  # both within the first (or the last) 30 rows
        rows = [int(x) for x in rng.choice(30, size=2, replace=False)]
        mismatch(read, win, c, rows if rng.random() < 0.5 else [n - 1 - r for r in rows])
    elif kind == "each_end":
        mismatch(read, win, c, [int(rng.integers(0, 30)), n - 1 - int(rng.integers(0, 30))])
    elif kind == "three_ag":  # three A read bases against G: deficit 3 x 326 = 978, J3 = 1
        mismatch(read, win, c, mid, 0, 2)
    elif kind == "end_copy":  # two mismatches in the first 10 rows, those rows copied to the window's start
        mismatch(read, win, c, [int(x) for x in rng.choice(10, size=2, replace=False)])
        at = int(rng.integers(0, 3))  # (column 0: item 6's case; columns 1 and 2: the path with three gap runs)
        if at + 12 < c:
            win[at:at + 12] = read[:12]
    elif kind == "indel":
        x = int(rng.integers(20, n - 20))
        read = np.concatenate([read[:x], read[x + 3:], rng.integers(0, 4, size=3).astype(np.uint8)])
    return np.ascontiguousarray(read), win


@functools.lru_cache(maxsize=None)
def batch(seed, count, kinds=KINDS, ms=None, ns=N_CHOICES):
    """(reads, windows, oracle result): computed once, shared, not to be changed"""
    rng = np.random.default_rng(seed)
    reads, wins = [], []
    for k in range(count):
        n = ns[k % len(ns)]
        mc = ms or m_choices(n)
        a, b = make_pair(rng, n, mc[(k // len(ns)) % len(mc)], kinds[(k // (len(ns) * len(mc))) % len(kinds)])
        reads.append(a); wins.append(b)
    return reads, wins, oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=8)


def test_mixed_batch(gpu_lib, monkeypatch):
    """every kind x every read length x windows of n + 2, 300 and 2 000 columns"""
    count = 2003
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(5100, count)
    cert, offered = base.run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "deficit, mixed")
    host = base.host_certified(monkeypatch, p, reads, wins)
    print("certified %d of %d (host %d)" % (cert, offered, host))
    assert offered == count and cert == host
    assert count // 6 < cert < count * 2 // 3  # (mid2, each_end and three_ag in the long windows; never end2, end_copy, indel)


def test_two_mid_read_mismatches_all_certified(gpu_lib, monkeypatch):
    """13 reads of 150 bases with two mid-read mismatches in 2 000-column windows: deficit 2 x 326 .. 2 x 446 > 600, all certified"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(5200, 13, kinds=("mid2",), ms=(2000,), ns=(150,))
    assert base.run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "deficit, mid") == (13, 13)


def test_head_mismatches_with_a_head_copy_none_certified(gpu_lib, monkeypatch):
    """the same 13 shapes with both mismatches in the first 10 rows and those rows copied to the window's start (column 0: item 6's
    case; columns 1 and 2: the path with three gap runs that the edge rule excludes): none certified, and the oracle's CIGARs, which are not
    the closed form, come out of the sweep"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(5300, 13, kinds=("end_copy",), ms=(2000,), ns=(150,))
    assert base.run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "deficit, head copy") == (0, 13)
