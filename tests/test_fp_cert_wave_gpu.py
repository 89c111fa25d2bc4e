"""The gapless certificate's decision spread over the wave (fp_cert.hip.h): a lane takes ceil(n / 64) consecutive rows, so
the read lengths here sit on the chunk-size boundaries (64 and 128 rows) and at both ends of the kernel's range.  With the certificate on
and off the results are the oracle's, bit for bit, and the kernel certifies exactly the pairs the host's serial decision certifies."""
import functools

import numpy as np
import pytest

import asym
import oracle
import test_fp_cert_cpu as cpu
import test_fp_cert_gpu as base
from gonomics_amd import align

pytestmark = pytest.mark.gpu

HCT = align.HumanChimpTwoScoreMatrix
GO, GE = -600, -150
NS = (16, 63, 64, 65, 66, 127, 128, 129, 150, 152, 153, 160)
KINDS = base.KINDS + ("edge", "tail_tie")
T1, T2 = 15, 30  # the edge rule's rows for K = 16 and two mismatches under HCT, gapOpen -600 (J3 = 0)


def make_pair(rng, n, m, kind):
    if kind == "indel" and n < 46:  # (base.make_pair cuts 20 bases in from either end)
        kind = "exact"
    if kind not in ("edge", "tail_tie"):
        return base.make_pair(rng, n, m, kind)
    read, win = base.make_pair(rng, n, m, "exact")
    c = next(c for c in range(m - n + 1) if np.array_equal(win[c:c + n], read)) if kind == "tail_tie" else None
    if kind == "edge":  # two mismatches on the rows T1 - 1 / T1 and T2 - 1 / T2 from either end
        rows = sorted({r % n for r in (T1 - 1, T1, T2 - 1, T2, n - T2 - 1, n - T2, n - T1 - 1, n - T1)})
        for x in rng.choice(rows, size=2, replace=False):
            read[int(x)] = (int(read[int(x)]) + int(rng.integers(1, 4))) % 4
    else:  # the last d bases also on the window's last columns, one of them a mismatch on the diagonal: G ties over several d
        d = int(rng.integers(2, min(12, n)))
        win[m - d:] = read[n - d:]
        x = n - d + int(rng.integers(0, d))
        if c + n <= m - d:
            win[c + x] = (int(win[c + x]) + int(rng.integers(1, 4))) % 4
    return np.ascontiguousarray(read), win


@functools.lru_cache(maxsize=None)
def batch(seed, count, matrix="HCT"):
    """(reads, windows, oracle result): computed once, shared, not to be changed"""
    mx = {"HCT": HCT, "ASYM": asym.ASYM, "BAD": cpu.BAD}[matrix]
    rng = np.random.default_rng(seed)
    reads, wins = [], []
    for k in range(count):
        n = NS[(k + seed) % len(NS)]
        m = (n + 2, 300, 2000)[(k // len(NS) + k) % 3]
        a, b = make_pair(rng, n, m, KINDS[(k // 2 + seed) % len(KINDS)])
        reads.append(a); wins.append(b)
    exp = oracle.align_batch(oracle.MODE_AFFINE, mx, GO, GE, reads, wins, threads=8)
    return mx, reads, wins, exp


def run(gpu_lib, monkeypatch, seed, count, matrix="HCT"):
    mx, reads, wins, exp = batch(seed, count, matrix)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, mx, GO, GE)
    cert, offered = base.run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "%s, %d pairs" % (matrix, count))
    host = base.host_certified(monkeypatch, p, reads, wins)
    print("%s, %d pairs: %d certified, the host certifies %d" % (matrix, count, cert, host))
    assert offered == count and cert == host, (cert, host, offered)
    return cert


@pytest.mark.parametrize("count", [1, 9, 257])
def test_batches(gpu_lib, monkeypatch, count):
    """every kind, every read length, windows of n + 2, 300 and 2 000 columns"""
    for seed in range(4) if count < 257 else (0,):
        cert = run(gpu_lib, monkeypatch, 5200 + seed, count)
    if count == 257:
        assert 40 <= cert <= 257 - 40


def test_asymmetric_matrix(gpu_lib, monkeypatch):
    """asym.ASYM (lambda = 111: K = 16 admits exact reads from 111 bases on)"""
    assert run(gpu_lib, monkeypatch, 5300, 257, "ASYM") > 10


def test_matrix_the_certificate_refuses(gpu_lib, monkeypatch):
    """BAD of tests/test_fp_cert_cpu.py (A against C scores like A against A): nothing is certified, nothing launched, same results"""
    assert run(gpu_lib, monkeypatch, 5400, 257, "BAD") == 0
