"""The fast path's gapless certificate on the device (fp_cert.hip.h): with the switch on and off the results are the
oracle's, bit for bit; the counters (gnx_debug_counter 9 / 10) are asserted where the construction of the batch decides them."""
import functools

import numpy as np
import pytest

import oracle
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu

HCT = align.HumanChimpTwoScoreMatrix
GO, GE = -600, -150
N_CHOICES = (46, 62, 66, 150, 152, 153, 160)
KINDS = ("exact", "tail", "head", "copy", "piece", "near_copy", "homopolymer", "tandem", "mismatch", "two_n", "read_n", "indel")


def m_choices(n):
    return (n + 1, n + 2, 300, 2000)


def make_pair(rng, n, m, kind):
    """(read, window) of one adversarial kind; the read sits in the interior when the window leaves room for one"""
    win = rng.integers(0, 4, size=m).astype(np.uint8)
    c = int(rng.integers(1, m - n)) if m - n >= 2 else 0
    if kind == "homopolymer":
        win[max(0, c - 5):c + n + 5] = int(rng.integers(0, 4))
    elif kind == "tandem":
        unit = rng.integers(0, 4, size=int(rng.integers(2, 7))).astype(np.uint8)
        win[max(0, c - 9):c + n + 9] = np.resize(unit, min(m, c + n + 9) - max(0, c - 9))
    read = win[c:c + n].copy()
    if kind == "tail":  # the last 1 .. 8 bases also equal the window's end
        d = int(rng.integers(1, 9))
        win[m - d:] = read[n - d:]
        read = win[c:c + n].copy()
    elif kind == "head":  # the first bases equal the window's start
        d = int(rng.integers(1, 9))
        win[:d] = read[:d]
        read = win[c:c + n].copy()
    elif kind in ("copy", "piece", "near_copy"):  # a second copy of the read, or of a 16 .. 60-base piece, elsewhere (exact or with 1 - 2 mismatches)
        L = n if kind != "piece" else int(rng.integers(16, min(60, n) + 1))
        q = int(rng.integers(0, n - L + 1))
        piece = read[q:q + L].copy()
        if kind == "near_copy" or rng.random() < 0.3:
            for _ in range(int(rng.integers(1, 3))):
                x = int(rng.integers(0, L))
                piece[x] = (int(piece[x]) + 1) % 4
        at = int(rng.integers(0, m - L + 1))
        win[at:at + L] = piece
    elif kind == "mismatch":
        x = int(rng.integers(0, n))
        read[x] = (int(read[x]) + int(rng.integers(1, 4))) % 4
    elif kind == "two_n":  # two mismatches against N in the window
        for x in rng.choice(n, size=2, replace=False):
            win[c + int(x)] = 4
    elif kind == "read_n":
        read[int(rng.integers(0, n))] = 4
    elif kind == "indel":
        x = int(rng.integers(20, n - 20))
        read = np.concatenate([read[:x], read[x + 3:], rng.integers(0, 4, size=3).astype(np.uint8)])
    return np.ascontiguousarray(read), win


@functools.lru_cache(maxsize=None)
def batch(seed, count, kinds=KINDS, ms=None, ns=N_CHOICES):
    """(reads, windows, oracle result, [(n, m, kind)]): computed once, shared, not to be changed"""
    rng = np.random.default_rng(seed)
    reads, wins, meta = [], [], []
    for k in range(count):
        n = ns[k % len(ns)]
        m = (ms or m_choices(n))[(k // len(ns)) % len(ms or m_choices(n))]
        kind = kinds[(k // 3) % len(kinds)]
        a, b = make_pair(rng, n, m, kind)
        reads.append(a); wins.append(b); meta.append((n, m, kind))
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=8)
    return reads, wins, exp, meta


# With K = 16, gapOpen -600 and this matrix (lambda = 296) the "K is long enough" rule admits exact reads from 63 bases on:
# J = 0, J1 = 2, 16 <= ceil(n / 3) and 16 <= ceil((n - 2) / 4).  So 46 and 62 are never certified, 66 and longer are.
N_CERTIFIABLE = (66, 150, 152, 153, 160)
SURE = ("exact", "tail", "head")  # kinds whose certificate the construction decides (a chance second 16-mer aside: ~1e-4 per pair)


def host_certified(monkeypatch, params, reads, wins):
    """how many of the pairs the host's certificate certifies (gnx_debug_gapless_certificate, K = 16 like the kernel): the kernel must
    certify exactly these -- a kernel that refused more would pass every parity check and only lose speed"""
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")
    return sum(1 for a, b in zip(reads, wins) if _lib.debug_gapless_certificate(params, a, b, K=16)[0])


def run_both(gpu_lib, monkeypatch, call, exp, what):
    """`call` with the certificate on (GNX_FP_CERT=2: whatever the batch size) and off: both the oracle's result; returns (certified,
    offered) of the run with it on"""
    from common import assert_same
    counts = None
    monkeypatch.setenv("GNX_FASTPATH", "2")  # no shape rules: windows of n + 1 columns and batches of one pair take the fast path too
    for sw in ("2", "0"):
        monkeypatch.setenv("GNX_FP_CERT", sw)
        gpu_lib.debug_counter(9); gpu_lib.debug_counter(10)
        got = call()
        assert gpu_lib.get_timing()["fast_path"] == 1
        assert_same(got, exp, "%s (GNX_FP_CERT=%s)" % (what, sw))
        c = (gpu_lib.debug_counter(9), gpu_lib.debug_counter(10))
        if sw == "2":
            counts = c
        else:
            assert c == (0, 0), c
    return counts


@pytest.mark.parametrize("count", [1, 7, 8, 9, 3003])
def test_mixed_batches(gpu_lib, monkeypatch, count):
    """every kind, every read length, windows of n + 1, n + 2, 300 and 2 000 columns in one batch"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp, meta = batch(4100 + count, count)
    cert, offered = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "mixed %d" % count)
    sure = sum(1 for n, m, kind in meta if kind in SURE and n in N_CERTIFIABLE and m >= 300)
    never = sum(1 for n, m, kind in meta if kind in ("indel", "read_n") or n < 63 or m < n + 2)
    assert offered == count and sure <= cert <= count - never, (cert, sure, never)
    assert cert == host_certified(monkeypatch, p, reads, wins)
    if count == 3003:
        assert sure > 100 and never > 1000 and (count - cert) % 8 != 0, (sure, never, cert)  # (a live list that ends inside a wave's eight pairs)


@pytest.mark.parametrize("count", [8, 13])
def test_everything_certified_or_nothing(gpu_lib, monkeypatch, count):
    """exact reads in the interior of random windows: the live list is empty; reads with an indel: it is everything"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp, _ = batch(4200 + count, count, kinds=SURE, ms=(300, 2000), ns=N_CERTIFIABLE)
    assert run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "all certified") == (count, count)
    reads, wins, exp, _ = batch(4300 + count, count, kinds=("indel", "read_n"), ms=(300, 2000))
    assert run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "none certified") == (0, count)


@pytest.mark.parametrize("checker", [7, 64])
def test_checkerboards_inside_the_matrix(gpu_lib, monkeypatch, checker):
    """certifiable reads under a checkerboard whose edges lie inside the matrix: the walk's quirks decide, nothing is certified"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE, checker, checker)
    reads, wins, _, _ = batch(4213, 13, kinds=SURE, ms=(300, 2000), ns=N_CERTIFIABLE)
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, checker, checker, threads=8)
    assert run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "checkerboard %d" % checker) == (0, 13)


def test_bad_byte_in_the_window(gpu_lib, monkeypatch):
    """a byte >= 5 in the window of an otherwise certifiable pair: the same error with the switch on and off"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, _, _ = batch(4208, 8, kinds=("exact",), ms=(300, 2000), ns=N_CERTIFIABLE)
    wins = [w.copy() for w in wins]
    wins[5][7] = 9
    monkeypatch.setenv("GNX_FASTPATH", "2")
    for sw in ("2", "0"):
        monkeypatch.setenv("GNX_FP_CERT", sw)
        with pytest.raises(gpu_lib.GnxError) as ei:
            gpu_lib.align_batch(p, list(reads), wins)
        assert ei.value.code == gpu_lib.GNX_EBASE


def test_packed_reference_and_sub_batches(gpu_lib, monkeypatch):
    """the packed resident reference (gnx_align_batch_by_offset) and a host-entry call cut into several sub-batches"""
    from common import assert_same
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    rng = np.random.default_rng(4400)
    ref = rng.integers(0, 4, size=30000).astype(np.uint8)
    ref[rng.integers(0, 30000, size=6)] = 4
    count = 203
    starts = rng.integers(0, 30000 - 2000, size=count).astype(np.int64)
    lens = np.asarray([(300, 2000, 1000, 777)[k % 4] for k in range(count)], dtype=np.int64)
    reads = []
    for k in range(count):
        n = N_CHOICES[k % len(N_CHOICES)]
        c = int(rng.integers(1, lens[k] - n))
        r = ref[starts[k] + c:starts[k] + c + n].copy()
        if k % 3 == 1:
            x = int(rng.integers(0, n))
            r[x] = (int(r[x]) + 1) % 4
        if k % 5 == 4:
            r = np.concatenate([r[:30], r[32:], r[:2]])
        reads.append(r)
    a_cat = np.concatenate(reads)
    a_off = np.zeros(count + 1, dtype=np.int64)
    a_off[1:] = np.cumsum([len(r) for r in reads])
    exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, [ref[s:s + l] for s, l in zip(starts, lens)], threads=8)
    gpu_lib.set_reference(ref)
    cert, offered = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch_by_offset(p, a_cat, a_off, starts, lens), exp, "packed reference")
    assert offered == count and 0 < cert < count  # (exact reads of 66 bases and more in windows without an N; reads with an indel)
    wins = [ref[s:s + l] for s, l in zip(starts, lens)]
    # the packed route refuses windows whose 64-base blocks hold an exception (an N here), whether or not the N lies inside the window
    clean = [not np.any(ref[(s >> 6) << 6:(((s + l - 1) >> 6) + 1) << 6] >= 4) for s, l in zip(starts, lens)]
    assert 0 < sum(clean) < count
    assert cert == host_certified(monkeypatch, p, [r for r, c in zip(reads, clean) if c], [w for w, c in zip(wins, clean) if c])
    monkeypatch.setenv("GNX_HOST_SUB", "64")
    a_len = np.diff(a_off)
    cert2, offered2 = run_both(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch_windows(p, a_cat, a_off[:-1], a_len, ref, starts, lens), exp, "sub-batches")
    assert offered2 == count and cert2 >= cert  # (byte windows: the windows with an N can be certified as well)
    assert cert2 == host_certified(monkeypatch, p, reads, wins)


def test_batch_size_rule(gpu_lib, monkeypatch):
    """without the switch the certificate runs for batches that fill the device more than once (8 pairs x 3 waves x 4 SIMDs per CU)
    and for no smaller one; results are the oracle's either way"""
    from common import assert_same
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    monkeypatch.delenv("GNX_FP_CERT", raising=False)
    fill = 8 * 3 * 4 * 256  # (the MI355X has 256 CUs)
    for count in (fill + 11, 64):
        reads, wins, exp, meta = batch(4500, count, kinds=SURE + ("indel",), ms=(800,), ns=(66,))
        gpu_lib.debug_counter(9); gpu_lib.debug_counter(10)
        assert_same(gpu_lib.align_batch(p, list(reads), list(wins)), exp, "batch of %d" % count)
        assert gpu_lib.get_timing()["fast_path"] == 1
        cert, offered = gpu_lib.debug_counter(9), gpu_lib.debug_counter(10)
        if count > fill:
            assert offered == count and cert == sum(1 for n, m, kind in meta if kind in SURE), (cert, offered)
        else:
            assert (cert, offered) == (0, 0)
