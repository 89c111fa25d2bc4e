"""The four-wave form of the headline sweep (fp_sweep_kernel<RR, XP, PK, 4>) on the device: with GNX_FP_WG4=2 (always) and
=0 (never) the results are the oracle's, bit for bit -- scores, offsets, run lengths, ops -- for byte windows, the packed resident
reference and the transposed local form, with the gapless certificate on and off, in one launch and split into rounds.

The batches are the smallest at which the form can go wrong.  Pair k sits in wave k // 8 of workgroup k // 32: batch sizes on the wave and
workgroup edges (a workgroup with three empty waves, a wave with one pair), reads of 1 .. 160 bases mixed in one batch (19 and 20 rows per
lane, fewer rows than planes), and windows of n + 2 .. 700 columns mixed inside one workgroup: a wave of windows under 16 columns with one
under 7 (it starts in the tagged tail) beside waves of 200 and of 700 columns, so the four waves end hundreds of steps apart."""
import functools

import numpy as np
import pytest

import common
import oracle
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu

HCT = align.HumanChimpTwoScoreMatrix
GO, GE = -600, -150
SIZES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100)
SPLIT_SIZES = (33, 64, 65, 96, 97, 129)
NS = (150, 2, 152, 19, 160, 66, 3, 153, 100, 20, 5, 159, 37, 151, 8, 64, 149, 21, 4, 76)


def make_pairs(seed, count, n_max):
    """(reads, windows): wave w = k // 8 has windows of class (w + seed) % 4 -- 0: n + 2 .. n + 9 columns and one pair of <= 4 bases in a
    window of <= 6; 1: about 200; 2: anything from n + 2 to 700; 3: 700.  Reads: copies of a piece of the window -- exact (the certificate
    takes the long ones), with substitutions and indels, or unrelated"""
    rng = np.random.default_rng(seed)
    reads, wins = [], []
    for k in range(count):
        w, q = k // 8, k % 8
        cls = (w + seed) % 4
        n = min(NS[(k * 7 + w) % len(NS)], n_max)
        if cls == 0:
            if q == 3 or count == 1:
                n = 1 + w % 4
            m = n + 2 + (q if q != 3 else 0)
        elif cls == 1:
            m = 200 + 13 * q
        elif cls == 2:
            m = (n + 2, 700, 333, n + 3, 512, n + 64, 699, n + 40)[q]
        else:
            m = 700 - k % 3
        m = max(m, n + 2)
        win = rng.integers(0, 4, size=m).astype(np.uint8)
        c = int(rng.integers(1, m - n))
        kind = rng.random()
        if kind < 0.3:
            read = win[c:c + n].copy()
        elif kind < 0.85:
            read = common.mutate(rng, win[c:c + n + 12], 0.04, 0.03, alphabet=4)[:n]
            if read.shape[0] < n:
                read = np.concatenate([read, rng.integers(0, 4, size=n - read.shape[0]).astype(np.uint8)])
        else:
            read = rng.integers(0, 4, size=n).astype(np.uint8)
        reads.append(np.ascontiguousarray(read)); wins.append(win)
    return reads, wins


@functools.lru_cache(maxsize=None)
def batch(count, n_max, local=False):
    """(reads, windows, the oracle's result): computed once, shared by the tests, not to be changed"""
    reads, wins = make_pairs(7000 + count + n_max, count, n_max)
    if local:
        exp = oracle.align_batch(oracle.MODE_AFFINE_LOCAL, HCT, GO, GE, wins, reads, threads=8)
    else:
        exp = oracle.align_batch(oracle.MODE_AFFINE, HCT, GO, GE, reads, wins, threads=8)
    return reads, wins, exp


def both_forms(gpu_lib, monkeypatch, call, exp, what, certs=("2", "0")):
    """`call` with the four-wave form forced and forbidden, the certificate forced and off: the oracle's result every time"""
    monkeypatch.setenv("GNX_FASTPATH", "2")  # no shape rules: the sweep for every batch size and window length
    for cert in certs:
        monkeypatch.setenv("GNX_FP_CERT", cert)
        for wg in ("2", "0"):
            monkeypatch.setenv("GNX_FP_WG4", wg)
            got = call()
            assert gpu_lib.get_timing()["fast_path"] == 1
            common.assert_same(got, exp, "%s (GNX_FP_WG4=%s, GNX_FP_CERT=%s)" % (what, wg, cert))


def test_the_batches_are_what_they_claim():
    reads, wins, _ = batch(100, 160)
    ns, ms = [len(r) for r in reads], [len(w) for w in wins]
    assert min(ns) == 1 and max(ns) == 160 and any(n < 4 for n in ns) and min(ms) < 7 and max(ms) == 700
    assert all(m >= n + 2 for n, m in zip(ns, ms))
    for g in range(0, 96, 32):  # every full workgroup: its waves' longest windows differ by hundreds of columns
        tops = [max(ms[g + 8 * w:g + 8 * w + 8]) for w in range(4)]
        assert max(tops) - min(tops) > 400, tops
    assert any(min(ms[w:w + 8]) < 7 for w in range(0, 96, 8))  # a wave that starts in the tagged tail
    assert max(len(r) for r in batch(100, 152)[0]) == 152


@pytest.mark.parametrize("n_max", [152, 160])
@pytest.mark.parametrize("count", SIZES)
def test_byte_windows(gpu_lib, monkeypatch, count, n_max):
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(count, n_max)
    both_forms(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "byte windows, %d pairs" % count)


@pytest.mark.parametrize("n_max", [152, 160])
@pytest.mark.parametrize("count", SIZES)
def test_packed_resident_reference(gpu_lib, monkeypatch, count, n_max):
    """the same pairs through gnx_align_batch_by_offset: the windows laid end to end are the reference (no N: every window stays packed)"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(count, n_max)
    ref = np.concatenate(wins)
    lens = np.asarray([len(w) for w in wins], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    a_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    gpu_lib.set_reference(ref)
    both_forms(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch_by_offset(p, np.concatenate(reads), a_off, starts, lens), exp, "packed reference, %d pairs" % count)


@pytest.mark.parametrize("n_max", [152, 160])
@pytest.mark.parametrize("count", SIZES)
def test_transposed_local(gpu_lib, monkeypatch, count, n_max):
    """AffineGapLocal(target = window, query = read): the transposed sweep (no certificate there)"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, HCT, GO, GE)
    reads, wins, exp = batch(count, n_max, local=True)
    both_forms(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(wins), list(reads)), exp, "local, %d pairs" % count, certs=("0",))


@pytest.mark.parametrize("round_wgs", ["1", "2", "3"])
@pytest.mark.parametrize("count", SPLIT_SIZES)
def test_split_launches(gpu_lib, monkeypatch, count, round_wgs):
    """GNX_FP_ROUND: rounds of one, two and three workgroups of 32 pairs, so that whole rounds and a remainder are two launches at these
    sizes (rounds of two: 65, 96 and 129 pairs; of three: 97 and 129; rounds of one are always whole): an exact multiple of a round and one
    pair either side of it; with the certificate the live list is what gets split"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, exp = batch(count, 160)
    monkeypatch.setenv("GNX_FP_ROUND", round_wgs)
    both_forms(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(p, list(reads), list(wins)), exp, "%d pairs, rounds of %s" % (count, round_wgs))
    pl = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, HCT, GO, GE)
    _, _, expl = batch(count, 160, local=True)
    both_forms(gpu_lib, monkeypatch, lambda: gpu_lib.align_batch(pl, list(wins), list(reads)), expl, "local, %d pairs, rounds of %s" % (count, round_wgs), certs=("0",))


@pytest.mark.parametrize("where", [5, 40, 64])
def test_bad_byte_in_a_window(gpu_lib, monkeypatch, where):
    """a byte >= 5 in one window (first workgroup; second wave of the second; the remainder launch): the one-wave form's error, same code"""
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, HCT, GO, GE)
    reads, wins, _ = batch(65, 160)
    wins = [w.copy() for w in wins]
    wins[where][len(wins[where]) // 2] = 9
    monkeypatch.setenv("GNX_FASTPATH", "2")
    monkeypatch.setenv("GNX_FP_CERT", "0")
    monkeypatch.setenv("GNX_FP_ROUND", "2")
    codes = []
    for wg in ("0", "2"):
        monkeypatch.setenv("GNX_FP_WG4", wg)
        with pytest.raises(gpu_lib.GnxError) as ei:
            gpu_lib.align_batch(p, list(reads), wins)
        codes.append(ei.value.code)
    assert codes == [gpu_lib.GNX_EBASE, gpu_lib.GNX_EBASE], codes
