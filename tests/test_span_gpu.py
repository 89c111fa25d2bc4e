"""AffineGapLocal's score, target start and target end without a CIGAR on the device (gnx_locate_span_*).  Every
comparison is exact equality of int64 values with what the oracle's AffineGapLocal gives: its score, the leading ColD run of its
CIGAR and the target length minus its trailing ColD run -- no tolerance, no case left out."""
import subprocess

import numpy as np
import pytest

import common
import oracle
import pyref_span
from gonomics_amd import align

pytestmark = pytest.mark.gpu
MX = common.matrices()
FLAT = pyref_span.FLAT


def _los(mx, go, ge, exp, queries):
    return np.asarray([pyref_span.window_lo(exp[0][p], exp[2][p], len(queries[p]), mx, go, ge) for p in range(len(queries))])


def _check_lists(L, mx, go, ge, targets, queries, route, what="", exp=None):
    """locate_span_batch == oracle; its score and end == locate_batch; its score == the align call's; route True: fast_path 10 ran"""
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
    if exp is None:
        exp = pyref_span.spans_from_oracle(mx, go, ge, targets, queries, threads=16)
    sc, st, en = L.locate_span_batch(p, targets, queries)
    fp = L.get_timing()["fast_path"]
    assert sc.dtype == np.int64 and st.dtype == np.int64 and en.dtype == np.int64
    assert np.array_equal(sc, exp[0]), (what, "score", np.flatnonzero(sc != exp[0])[:8])
    assert np.array_equal(en, exp[2]), (what, "end", np.flatnonzero(en != exp[2])[:8])
    bad = np.flatnonzero(st != exp[1])
    assert bad.size == 0, (what, "start", bad[:8], st[bad][:8], exp[1][bad][:8])
    lsc, len_ = L.locate_batch(p, targets, queries)
    assert np.array_equal(sc, lsc) and np.array_equal(en, len_), what
    assert np.array_equal(sc, L.align_batch(p, targets, queries)[0]), what
    assert (fp == 10) if route else (fp != 10), (what, fp)
    return exp


@pytest.mark.parametrize("mname", sorted(MX))
def test_fuzz(gpu_lib, mname):
    """random_pairs with N bases, target and query 1 .. 400: target shorter than query, target of one base, query of one base"""
    targets, queries = common.random_pairs(700, 260, 1, 400, 1, 400)
    one = np.zeros(1, dtype=np.uint8)
    targets += [one, np.asarray([3], np.uint8), targets[0], one]
    queries += [queries[1], np.asarray([3], np.uint8), one, one + 2]
    assert any(len(t) < len(q) for t, q in zip(targets, queries))
    exp = _check_lists(gpu_lib, MX[mname], -400, -30, targets, queries, route=True, what="fuzz " + mname)
    assert np.any(exp[1] > 0) and np.any(exp[1] == 0)


def test_block_and_strip_edges(gpu_lib, monkeypatch):
    """query lengths around the 192-column strips of stage 2 (64 lanes x 3 columns), its lanes' column triples and the 160-row blocks
    of the sweep, against short and long targets"""
    rng = np.random.default_rng(17)
    targets, queries = [], []
    for ql in (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 159, 160, 161, 190, 191, 192, 193, 194, 320, 383, 384, 385, 700, 1024):
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
    exp = _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="edges")
    assert np.any(exp[1] > 0)
    monkeypatch.setenv("GNX_NO_PIPE", "1")
    _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="edges, one launch per level", exp=exp)


def test_window_arithmetic(gpu_lib):
    rng = np.random.default_rng(29)
    mx, go, ge = MX["Default"], -400, -30
    t = rng.integers(0, 4, size=10000).astype(np.uint8)
    s = rng.integers(0, 4, size=90).astype(np.uint8)
    L = 100  # one long deletion: the read is two pieces of the target 100 bases apart
    gapped = np.concatenate([t[6000:6075], t[6075 + L:6150 + L]])
    targets = [t, t, t, t, s, t[:300]]
    queries = [t[:150].copy(), t[-150:].copy(), t[5000:5150].copy(), gapped, rng.integers(0, 4, size=200).astype(np.uint8), t[:150].copy()]
    exp = _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="window arithmetic")
    assert (exp[1][0], exp[2][0]) == (0, 150) and (exp[1][1], exp[2][1]) == (9850, 10000) and (exp[1][2], exp[2][2]) == (5000, 5150)
    assert (exp[1][3], exp[2][3]) == (6000, 6150 + L)
    lo = _los(mx, go, ge, exp, queries)
    dmax = exp[2] - np.asarray([len(q) for q in queries]) - lo
    assert lo[0] == 0 and lo[2] > 4000 and lo[4] == 0 and np.any(lo > 0) and np.any(lo == 0), lo
    assert L <= dmax[3] <= L + 40, (dmax, lo)  # the route's deletion uses most of what the bound allows


@pytest.mark.parametrize("go,ge", [(0, -30), (-400, 0), (0, 0), (-7, -3)])
def test_ties_and_degenerate_penalties(gpu_lib, go, ge):
    rng = np.random.default_rng(11)
    targets = [np.full(n, b, np.uint8) for n, b in ((1, 0), (400, 0), (150, 2), (500, 2), (320, 0), (77, 4), (9, 0))]
    queries = [np.full(m, b, np.uint8) for m, b in ((9, 0), (17, 0), (160, 2), (161, 2), (333, 3), (40, 4), (1, 0))]
    targets += [rng.integers(0, 2, size=n).astype(np.uint8) for n in (300, 190, 322, 50, 700)]
    queries += [rng.integers(0, 2, size=m).astype(np.uint8) for m in (50, 200, 321, 300, 65)]
    for mx in (MX["Default"], FLAT):
        exp = _check_lists(gpu_lib, mx, go, ge, targets, queries, route=True, what="ties %d %d" % (go, ge))  # (gapExtend == 0: still route 10)
        if ge == 0:
            assert np.all(_los(mx, go, ge, exp, queries) == 0)
        assert np.any(exp[1] > 0)


def test_windows_and_resident_reference(gpu_lib):
    mx, go, ge = MX["HumanChimpTwo"], -600, -150
    n = 600
    reads, chunk = common.c2_workload(23, n, read_len=300, chunk_len=10000)
    chunk = chunk.copy()
    chunk[4096:4096 + 200] = 4  # an N block: windows that touch it read the exception list of the packed reference
    rng = np.random.default_rng(5)
    lens = np.where(rng.random(n) < 0.5, rng.integers(1, 65, size=n), rng.integers(65, 301, size=n)).astype(np.int64)
    q = reads.reshape(-1)
    q_start = np.arange(n, dtype=np.int64) * 300
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
    # _windows: every read against the whole shared chunk
    t_start, t_len = np.zeros(n, dtype=np.int64), np.full(n, chunk.shape[0], dtype=np.int64)
    exp = pyref_span.spans_from_oracle(mx, go, ge, [chunk] * n, [q[s:s + l] for s, l in zip(q_start, lens)], threads=16)
    sc, st, en = gpu_lib.locate_span_batch_windows(p, chunk, t_start, t_len, q, q_start, lens)
    assert gpu_lib.get_timing()["fast_path"] == 10
    assert np.array_equal(sc, exp[0]) and np.array_equal(st, exp[1]) and np.array_equal(en, exp[2]), np.flatnonzero(st != exp[1])[:8]
    # the resident reference (packed 2 bit) as the target: windows at odd offsets, some on the N block, some shorter than their read
    cat = np.concatenate([q[s:s + l] for s, l in zip(q_start, lens)])
    q_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r_len = rng.integers(1, 3001, size=n).astype(np.int64)
    r_start = rng.integers(0, chunk.shape[0] - 3000, size=n).astype(np.int64)
    r_start[::7] = 4001
    r_start[1::7] = 3000 + rng.integers(0, 1000, size=r_start[1::7].shape[0])
    r_len[1::7] = 3000  # long windows that end past the N block: some trimmed windows [lo, end) touch it, some do not
    assert np.any(r_start % 4 != 0) and np.any(r_start % 32 != 0) and np.any(r_start % 64 != 0) and np.any(r_len < lens)
    windows = [chunk[s:s + l] for s, l in zip(r_start, r_len)]
    queries = [cat[q_off[k]:q_off[k + 1]] for k in range(n)]
    exp = pyref_span.spans_from_oracle(mx, go, ge, windows, queries, threads=16)
    lo = _los(mx, go, ge, exp, queries)
    touch_full = (r_start < 4296) & (r_start + r_len > 4096)
    touch_trim = (r_start + lo < 4296) & (r_start + exp[2] > 4096)
    assert np.any(touch_trim) and np.any(touch_full & ~touch_trim)
    gpu_lib.set_reference(chunk)
    try:
        sc, st, en = gpu_lib.locate_span_batch_by_offset(p, cat, q_off, r_start, r_len)
        assert gpu_lib.get_timing()["fast_path"] == 10
        assert np.array_equal(sc, exp[0]), np.flatnonzero(sc != exp[0])[:8]
        assert np.array_equal(en, exp[2]), np.flatnonzero(en != exp[2])[:8]
        assert np.array_equal(st, exp[1]), (np.flatnonzero(st != exp[1])[:8], st[st != exp[1]][:8], exp[1][st != exp[1]][:8])
        lsc, len_ = gpu_lib.locate_batch_by_offset(p, cat, q_off, r_start, r_len)
        assert np.array_equal(sc, lsc) and np.array_equal(en, len_)
        # a base >= 5 in a read, and one in a touched window: GNX_EBASE, as the align twin
        bad_cat = cat.copy()
        bad_cat[q_off[3] + 1 if lens[3] > 1 else q_off[3]] = 7
        for fn in (gpu_lib.locate_span_batch_by_offset, gpu_lib.align_batch_by_offset):
            with pytest.raises(gpu_lib.GnxError) as ei:
                fn(p, bad_cat, q_off, r_start, r_len)
            assert ei.value.code == gpu_lib.GNX_EBASE
        bad_chunk = chunk.copy()
        bad_chunk[4100] = 6
        gpu_lib.set_reference(bad_chunk)
        for fn in (gpu_lib.locate_span_batch_by_offset, gpu_lib.align_batch_by_offset):
            with pytest.raises(gpu_lib.GnxError) as ei:
                fn(p, cat, q_off, r_start, r_len)
            assert ei.value.code == gpu_lib.GNX_EBASE
        untouched = (r_start + r_len <= 4100) | (r_start > 4100)
        keep = np.flatnonzero(untouched)[:50]
        k_off = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
        k_cat = np.concatenate([cat[q_off[k]:q_off[k + 1]] for k in keep])
        sc, st, en = gpu_lib.locate_span_batch_by_offset(p, k_cat, k_off, r_start[keep], r_len[keep])
        assert np.array_equal(sc, exp[0][keep]) and np.array_equal(st, exp[1][keep]) and np.array_equal(en, exp[2][keep])
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def test_fallbacks(gpu_lib, monkeypatch):
    """everything route 10 does not take runs the align route, with start and end read off its CIGAR on the device"""
    rng = np.random.default_rng(41)
    t, q = common.random_pairs(43, 24, 1, 300, 1, 300)
    e = np.zeros(0, dtype=np.uint8)
    mx = MX["Default"]
    _check_lists(gpu_lib, mx, 25, -30, t, q, route=False, what="gapOpen > 0")
    _check_lists(gpu_lib, mx, -400, 5, t, q, route=False, what="gapExtend > 0")
    exp = _check_lists(gpu_lib, mx, -400, -30, t[:20] + [e, t[3], e], q[:20] + [q[2], e, e], route=False, what="empty sequences")
    assert [(int(exp[1][k]), int(exp[2][k])) for k in (20, 21, 22)] == [(0, 0)] * 3  # empty target, empty query, both empty
    long_q = rng.integers(0, 4, size=10241).astype(np.uint8)
    _check_lists(gpu_lib, mx, -400, -30, [t[0], long_q[5000:5060]], [q[0], long_q], route=False, what="a query past 10 240 bases (the bound of route 10)")
    big = (np.asarray(mx, dtype=np.int64) * 100000).tolist()
    _check_lists(gpu_lib, big, -400 * 100000, -30 * 100000, t, q, route=False, what="beyond int32")
    exp = _check_lists(gpu_lib, mx, -400, -30, t, q, route=True, what="route 10")
    monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
    _check_lists(gpu_lib, mx, -400, -30, t, q, route=False, what="GNX_SCORE_SWEEP=0", exp=exp)


def test_two_contexts_on_one_device(gpu_lib, monkeypatch):
    L = gpu_lib.lib()
    targets, queries = common.random_pairs(82, 240, 1, 900, 1, 500)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, MX["Default"], -400, -30)
    one = gpu_lib.locate_span_batch(p, targets, queries)
    assert gpu_lib.get_timing()["fast_path"] == 10
    exp = pyref_span.spans_from_oracle(MX["Default"], -400, -30, targets, queries, threads=16)
    assert all(np.array_equal(a, b) for a, b in zip(one, exp))
    try:
        gpu_lib.check(L.gnx_shutdown() or 0)
        monkeypatch.setenv("GNX_RCCL", "0")
        assert gpu_lib.init_devices([0, 0], 8 << 30) == 2
        two = gpu_lib.locate_span_batch(p, targets, queries)
        tm = gpu_lib.get_timing()
        assert all(np.array_equal(a, b) for a, b in zip(two, one))
        assert tm["n_contexts"] == 2 and tm["fast_path"] == 10
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
    start = route[0].RunLength if route[0].Op == align.ColD and len(route) > 1 else 0
    end = len(t) - (route[-1].RunLength if route[-1].Op == align.ColD else 0)
    assert align.AffineGapLocalSpan(t, q, mx, -400, -30) == (score, start, end)
    assert 0 < start < end < len(t)
    sc, starts, ends = align.LocateSpanBatch(gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, mx, -400, -30), [t, q], [q, t])
    assert (sc[0], starts[0], ends[0]) == (score, start, end)
    with pytest.raises(gpu_lib.GnxError) as ei:
        align.LocateSpanBatch(gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, mx, -400, -30), [t], [q])
    assert ei.value.code == gpu_lib.GNX_EINVAL


def test_cpp_span_mirror_runs():
    import test_span_cpu
    test_span_cpu._build_cpp()
    assert subprocess.call([test_span_cpu.BIN]) == 0
