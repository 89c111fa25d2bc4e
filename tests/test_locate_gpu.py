"""AffineGapLocal's score and target end without a CIGAR on the device (gnx_score_* with mode 3 on the local sweep, gnx_locate_*).
Every comparison is exact equality of int64 values with what the oracle's AffineGapLocal gives: its score, and the target length
minus the trailing ColD run of its CIGAR -- no tolerance, no case left out."""
import os
import subprocess

import numpy as np
import pytest

import common
import oracle
from gonomics_amd import align

pytestmark = pytest.mark.gpu
MX = common.matrices()
FLAT = [[1, -1, -1, -1, 0]] * 4 + [[0, 0, 0, 0, 0]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ends(ops, off, target_lens):
    """target length minus the run length of the CIGAR's last op when that op is ColD"""
    ends = np.asarray(target_lens, dtype=np.int64).copy()
    for k in range(len(ends)):
        if off[k + 1] > off[k] and ops["op"][off[k + 1] - 1] == 2:
            ends[k] -= ops["run_length"][off[k + 1] - 1]
    return ends


def _expected(mx, go, ge, targets, queries, threads=16):
    sc, ops, off = oracle.align_batch(3, mx, go, ge, targets, queries, threads=threads)
    return sc, _ends(ops, off, [len(t) for t in targets])


def _check_lists(L, mx, go, ge, targets, queries, route, what="", exp=None):
    """score_batch (mode 3) and locate_batch == oracle == the align call's score; route True: the local sweep ran, False: it did not"""
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
    exp_s, exp_e = exp if exp is not None else _expected(mx, go, ge, targets, queries)
    got = L.score_batch(p, targets, queries)
    fp_score = L.get_timing()["fast_path"]
    sc, ends = L.locate_batch(p, targets, queries)
    fp_loc = L.get_timing()["fast_path"]
    assert got.dtype == np.int64 and sc.dtype == np.int64 and ends.dtype == np.int64
    assert np.array_equal(got, exp_s), (what, "score_batch", np.flatnonzero(got != exp_s)[:8])
    assert np.array_equal(sc, exp_s), (what, "locate score", np.flatnonzero(sc != exp_s)[:8])
    assert np.array_equal(ends, exp_e), (what, "end", np.flatnonzero(ends != exp_e)[:8], ends[ends != exp_e][:8], exp_e[ends != exp_e][:8])
    assert np.array_equal(got, L.align_batch(p, targets, queries)[0]), what
    if route:
        assert fp_score == 8 and fp_loc == 8, (what, fp_score, fp_loc)
    else:
        assert fp_score != 8 and fp_loc != 8, (what, fp_score, fp_loc)
    return exp_s, exp_e


@pytest.mark.parametrize("mname", sorted(MX))
def test_fuzz(gpu_lib, mname):
    """random_pairs with N bases, target and query 1 .. 400: target shorter than query, target of one base, query of one base"""
    targets, queries = common.random_pairs(700, 260, 1, 400, 1, 400)
    one = np.zeros(1, dtype=np.uint8)
    targets += [one, np.asarray([3], np.uint8), targets[0], one]
    queries += [queries[1], np.asarray([3], np.uint8), one, one + 2]
    assert any(len(t) < len(q) for t, q in zip(targets, queries))
    exp_s, exp_e = _check_lists(gpu_lib, MX[mname], -400, -30, targets, queries, route=True, what="fuzz " + mname)
    assert np.any(exp_e < np.asarray([len(t) for t in targets]))  # (ends inside the target are covered)


def test_block_edges(gpu_lib, monkeypatch):
    """query lengths around one, two and several row blocks (padding of 0 and 159 slots) against short and long targets in one batch"""
    rng = np.random.default_rng(17)
    targets, queries = [], []
    for ql in (1, 159, 160, 161, 319, 320, 321, 700):
        for tl in (1, 150, 700, 3000):
            t = rng.integers(0, 5, size=tl).astype(np.uint8)
            if tl >= ql and tl > 1:  # a related pair: the query is a mutated piece of the target
                o = int(rng.integers(0, tl - ql + 1))
                q = common.mutate(rng, t[o:o + ql], sub=0.05, indel=0.03, geo=0.4, alphabet=5)
                q = np.concatenate([q, rng.integers(0, 4, size=ql).astype(np.uint8)])[:ql]
            else:
                q = rng.integers(0, 5, size=ql).astype(np.uint8)
            targets.append(t)
            queries.append(q)
    mx, go, ge = MX["HumanChimpTwo"], -600, -150
    exp = _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="block edges")
    monkeypatch.setenv("GNX_NO_PIPE", "1")
    _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="block edges, one launch per level", exp=exp)


@pytest.mark.parametrize("go,ge", [(0, -30), (-400, 0), (0, 0), (-7, -3)])
def test_ties_and_degenerate_penalties(gpu_lib, go, ge):
    rng = np.random.default_rng(11)
    targets = [np.full(n, b, np.uint8) for n, b in ((1, 0), (400, 0), (150, 2), (500, 2), (320, 0), (77, 4), (9, 0))]
    queries = [np.full(m, b, np.uint8) for m, b in ((9, 0), (17, 0), (160, 2), (161, 2), (333, 3), (40, 4), (1, 0))]
    targets += [rng.integers(0, 2, size=n).astype(np.uint8) for n in (300, 190, 322, 50)]
    queries += [rng.integers(0, 2, size=m).astype(np.uint8) for m in (50, 200, 321, 300)]
    for mx in (MX["Default"], FLAT):
        exp_s, exp_e = _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="ties %d %d" % (go, ge))
        assert np.any(exp_e == np.asarray([len(t) for t in targets]))  # an end at the end of the target


def test_end_zero_and_end_at_target_length(gpu_lib):
    """Ends at both extremes.  With both sequences non-empty the end is never 0: I(i, m) >= gapOpen + m * gapExtend on every target
    row i >= 1 (I(i, 1) opens from the free D(i, 0) = 0), which is what the all-insertion start I(0, m) scores, and a tie goes to the
    LAST row -- so a query that mismatches the whole target under free gaps ends at n, not at 0.  The end is 0 exactly when the query
    (or the target) is empty: the route is the target's length of ColD, and such a batch takes the align route.  Also: an exact
    prefix ends right behind it, an exact suffix at n."""
    t = np.full(60, 0, np.uint8)
    rnd = np.random.default_rng(3).integers(0, 4, size=200).astype(np.uint8)
    e = np.zeros(0, np.uint8)
    targets, queries = [t, rnd, t, rnd], [np.full(20, 1, np.uint8), rnd[-50:].copy(), np.full(200, 1, np.uint8), rnd[:50].copy()]
    exp_s, exp_e = _check_lists(gpu_lib, MX["Default"], 0, 0, targets, queries, route=True, what="free gaps")
    assert exp_e[0] == 60 and exp_e[2] == 60, exp_e  # all-insertion start and every later row tie: the last one wins
    exp_s, exp_e = _check_lists(gpu_lib, MX["Default"], -400, -30, targets, queries, route=True, what="prefix / suffix")
    assert exp_e[1] == 200 and exp_e[3] == 50, exp_e
    for go, ge in ((0, 0), (-400, -30)):
        exp_s, exp_e = _check_lists(gpu_lib, MX["Default"], go, ge, targets + [t, e], queries + [e, queries[0]], route=False, what="end 0")
        assert exp_e[4] == 0 and exp_e[5] == 0 and exp_s[4] == 0, (exp_s, exp_e)


def _c2_mixed(seed, n_pairs, chunk_len=10000):
    """C2 shape with reads of 1 .. 160 and of 161 .. 700 bases in one batch (one, two and several row blocks)"""
    reads, chunk = common.c2_workload(seed, n_pairs, read_len=700, chunk_len=chunk_len)
    rng = np.random.default_rng(seed + 1)
    q_len = np.where(rng.random(n_pairs) < 0.5, rng.integers(1, 161, size=n_pairs), rng.integers(161, 701, size=n_pairs)).astype(np.int64)
    q_len[:4] = (1, 160, 161, 700)
    q_start = np.arange(n_pairs, dtype=np.int64) * 700
    t_start = np.zeros(n_pairs, dtype=np.int64)
    t_len = np.full(n_pairs, chunk_len, dtype=np.int64)
    return reads.reshape(-1), q_start, q_len, chunk.copy(), t_start, t_len


def test_windows_and_resident_reference(gpu_lib):
    mx, go, ge = MX["HumanChimpTwo"], -600, -150
    q, q_start, q_len, chunk, t_start, t_len = _c2_mixed(23, 2400)
    chunk[4096:4096 + 200] = 4  # an N block: windows that touch it read the exception list of the packed reference
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
    es, eops, eoff = oracle.align_batch_windows(3, mx, go, ge, chunk, t_start, t_len, q, q_start, q_len, threads=16)
    sc, ends = gpu_lib.locate_batch_windows(p, chunk, t_start, t_len, q, q_start, q_len)
    assert gpu_lib.get_timing()["fast_path"] == 8
    assert np.array_equal(sc, es), np.flatnonzero(sc != es)[:8]
    exp_e = _ends(eops, eoff, t_len)
    assert np.array_equal(ends, exp_e), np.flatnonzero(ends != exp_e)[:8]
    got = gpu_lib.score_batch_windows(p, chunk, t_start, t_len, q, q_start, q_len)
    assert gpu_lib.get_timing()["fast_path"] == 8 and np.array_equal(got, es)
    # the resident reference (packed 2 bit) as the target: windows of 1 .. 3 000 bases, some on the N block, some shorter than their read
    rng = np.random.default_rng(5)
    n = 600
    lens = q_len[:n]
    cat = np.concatenate([q[s:s + l] for s, l in zip(q_start[:n], lens)])
    q_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r_len = rng.integers(1, 3001, size=n).astype(np.int64)
    r_start = rng.integers(0, chunk.shape[0] - 3000, size=n).astype(np.int64)
    r_start[::7] = 4000
    assert np.any(r_len < lens)
    es, eops, eoff = oracle.align_batch_windows(3, mx, go, ge, chunk, r_start, r_len, cat, q_off[:-1], lens, threads=16)
    exp_e = _ends(eops, eoff, r_len)
    gpu_lib.set_reference(chunk)
    try:
        sc, ends = gpu_lib.locate_batch_by_offset(p, cat, q_off, r_start, r_len)
        assert gpu_lib.get_timing()["fast_path"] == 8
        assert np.array_equal(sc, es), np.flatnonzero(sc != es)[:8]
        assert np.array_equal(ends, exp_e), np.flatnonzero(ends != exp_e)[:8]
        # a base >= 5 in a read, and one in a touched window: GNX_EBASE, as the align twin
        bad_cat = cat.copy()
        bad_cat[q_off[3] + 1] = 7
        for fn in (gpu_lib.locate_batch_by_offset, gpu_lib.align_batch_by_offset):
            with pytest.raises(gpu_lib.GnxError) as ei:
                fn(p, bad_cat, q_off, r_start, r_len)
            assert ei.value.code == gpu_lib.GNX_EBASE
        bad_chunk = chunk.copy()
        bad_chunk[4100] = 6
        gpu_lib.set_reference(bad_chunk)
        for fn in (gpu_lib.locate_batch_by_offset, gpu_lib.align_batch_by_offset):
            with pytest.raises(gpu_lib.GnxError) as ei:
                fn(p, cat, q_off, r_start, r_len)
            assert ei.value.code == gpu_lib.GNX_EBASE
        untouched = (r_start + r_len <= 4100) | (r_start > 4100)
        keep = np.flatnonzero(untouched)[:50]
        k_off = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
        k_cat = np.concatenate([cat[q_off[k]:q_off[k + 1]] for k in keep])
        sc, ends = gpu_lib.locate_batch_by_offset(p, k_cat, k_off, r_start[keep], r_len[keep])
        assert np.array_equal(sc, es[keep]) and np.array_equal(ends, exp_e[keep])
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def test_fallbacks(gpu_lib, monkeypatch):
    """everything the local sweep does not take runs the align route, with the end read off its CIGAR on the device"""
    rng = np.random.default_rng(41)
    t, q = common.random_pairs(43, 24, 1, 300, 1, 300)
    e = np.zeros(0, dtype=np.uint8)
    mx = MX["Default"]
    _check_lists(gpu_lib, mx, 25, -30, t, q, route=False, what="gapOpen > 0")
    _check_lists(gpu_lib, mx, -400, 5, t, q, route=False, what="gapExtend > 0")
    exp_s, exp_e = _check_lists(gpu_lib, mx, -400, -30, t[:20] + [e, t[3], e], q[:20] + [q[2], e, e], route=False, what="empty sequences")
    assert exp_e[21] == 0 and exp_e[20] == 0 and exp_e[22] == 0  # an empty query gives end 0
    long_q = rng.integers(0, 4, size=10241).astype(np.uint8)
    _check_lists(gpu_lib, mx, -400, -30, [t[0], long_q[5000:5060]], [q[0], long_q], route=False, what="a query past 64 row blocks")
    big = (np.asarray(mx, dtype=np.int64) * 100000).tolist()
    _check_lists(gpu_lib, big, -400 * 100000, -30 * 100000, t, q, route=False, what="beyond int32")
    exp = _check_lists(gpu_lib, mx, -400, -30, t, q, route=True, what="the sweep")
    monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
    _check_lists(gpu_lib, mx, -400, -30, t, q, route=False, what="GNX_SCORE_SWEEP=0", exp=exp)


def test_two_contexts_on_one_device(gpu_lib, monkeypatch):
    L = gpu_lib.lib()
    targets, queries = common.random_pairs(82, 240, 1, 900, 1, 500)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, MX["Default"], -400, -30)
    one_s, one_e = gpu_lib.locate_batch(p, targets, queries)
    assert gpu_lib.get_timing()["fast_path"] == 8
    exp_s, exp_e = _expected(MX["Default"], -400, -30, targets, queries)
    assert np.array_equal(one_s, exp_s) and np.array_equal(one_e, exp_e)
    try:
        gpu_lib.check(L.gnx_shutdown() or 0)
        monkeypatch.setenv("GNX_RCCL", "0")
        assert gpu_lib.init_devices([0, 0], 8 << 30) == 2
        two_s, two_e = gpu_lib.locate_batch(p, targets, queries)
        tm = gpu_lib.get_timing()
        assert np.array_equal(two_s, one_s) and np.array_equal(two_e, one_e)
        assert tm["n_contexts"] == 2 and tm["fast_path"] == 8
    finally:
        monkeypatch.delenv("GNX_RCCL", raising=False)
        L.gnx_shutdown()
        gpu_lib.check(L.gnx_init(0, 8 << 30))


def test_python_one_pair_functions(gpu_lib):
    rng = np.random.default_rng(61)
    t = rng.integers(0, 4, size=900).astype(np.uint8)
    q = common.mutate(rng, t[300:520], sub=0.05, indel=0.02)
    mx = MX["Default"]
    score, route = align.AffineGapLocal(t, q, mx, -400, -30)
    end = len(t) - (route[-1].RunLength if route[-1].Op == align.ColD else 0)
    assert align.AffineGapLocalEnd(t, q, mx, -400, -30) == (score, end)
    assert 0 < end < len(t)
    sc, ends = align.LocateBatch(gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, mx, -400, -30), [t, q], [q, t])
    assert (sc[0], ends[0]) == (score, end)
    s2, r2 = align.AffineGapLocal(q, t, mx, -400, -30)
    assert (sc[1], ends[1]) == (s2, len(q) - (r2[-1].RunLength if r2[-1].Op == align.ColD else 0))
    with pytest.raises(gpu_lib.GnxError) as ei:
        align.LocateBatch(gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, mx, -400, -30), [t], [q])
    assert ei.value.code == gpu_lib.GNX_EINVAL


def test_cpp_locate_mirror_runs():
    import test_locate_cpu
    test_locate_cpu._build_cpp()
    assert subprocess.call([test_locate_cpu.BIN]) == 0
