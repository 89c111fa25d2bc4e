"""Paired-end placement (gnx_best_pair_windows / gnx_best_pair_by_offset, align.MapBestPair / align.MapReadPairs).
Expected values come from the CPU oracle on the FLATTENED pair list (AffineGapLocal, target = window, query = the read or its reverse
complement): score, start = the leading ColD run, end = the length minus the trailing ColD run.  They go through the restatement of the
selection rule (tests/pyref_pairs.py); the winners' CIGARs come from the same oracle call.  Every comparison is exact equality."""
import ctypes
import functools

import numpy as np
import pytest

import asym
import common
import oracle
import pyref_pairs
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu
MX = common.matrices()
LOCAL, COL_D = 3, 2
GO, GE = -400, -30
I64_MIN = np.iinfo(np.int64).min


def _rc(x):
    x = np.asarray(x, np.uint8)[::-1].copy()
    m = x < 4
    x[m] = 3 - x[m]
    return x


def _flatten(reads, target, cands):
    """(targets, queries) of the contract's pair list"""
    ts, qs = [], []
    for rd, cs in zip(reads, cands):
        for s, l, st in cs:
            ts.append(np.asarray(target[s:s + l], np.uint8))
            qs.append(_rc(rd) if st else np.asarray(rd, np.uint8))
    return ts, qs


def _expected(mx, go, ge, reads, target, cands, lo, hi, pen, ci=10000, res=None):
    ts, qs = _flatten(reads, target, cands)
    if res is None:
        res = oracle.align_batch(LOCAL, mx, go, ge, ts, qs, ci, ci, threads=16) if ts else (np.zeros(0, np.int64), np.zeros(0, oracle.CIGAR_DTYPE), np.zeros(1, np.int64))
    sc, ops, off = res
    nc, n = len(ts), len(reads)
    routes = [[(int(x), int(o)) for x, o in zip(ops["run_length"][off[c]:off[c + 1]], ops["op"][off[c]:off[c + 1]])] for c in range(nc)]
    start, end = np.zeros(nc, np.int64), np.zeros(nc, np.int64)
    for c, rt in enumerate(routes):
        end[c] = len(ts[c]) - (rt[-1][0] if rt and rt[-1][1] == COL_D else 0)
        start[c] = rt[0][0] if len(rt) > 1 and rt[0][1] == COL_D else 0
    flat = [cd for cs in cands for cd in cs]
    c_off = np.concatenate([[0], np.cumsum([len(cs) for cs in cands])]).astype(np.int64)
    tables = [[(int(sc[c]), flat[c][0] + int(start[c]), flat[c][0] + int(end[c]), flat[c][2]) for c in range(c_off[r], c_off[r + 1])] for r in range(n)]
    best, second, proper, tlen = pyref_pairs.select_all(tables, lo, hi, pen)
    exp = {"cand_score": np.asarray(sc, np.int64)[:nc], "cand_start": start, "cand_end": end, "best": np.asarray(best, np.int32), "second_score": np.asarray(second, np.int64),
           "proper": np.asarray(proper, np.uint8), "tlen": np.asarray(tlen, np.int64), "score": np.zeros(n, np.int64), "target_start": np.zeros(n, np.int64),
           "target_end": np.zeros(n, np.int64), "routes": [[] for _ in range(n)], "tables": tables, "c_off": c_off}
    for r in range(n):
        if best[r] >= 0:
            c = c_off[r] + best[r]
            exp["score"][r], exp["target_start"][r], exp["target_end"][r], exp["routes"][r] = sc[c], start[c], end[c], routes[c]
    return exp


def _tables(reads, cands):
    r_cat = np.concatenate([np.asarray(r, np.uint8) for r in reads] + [np.zeros(1, np.uint8)])
    r_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    c_off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
    flat = [c for cs in cands for c in cs]
    return r_cat, r_off, c_off, [c[0] for c in flat], [c[1] for c in flat], [c[2] for c in flat]


def _call(L, p, reads, target, cands, lo, hi, pen, cigar=True, resident=False):
    r_cat, r_off, c_off, st, ln, sd = _tables(reads, cands)
    o = L.pair_opts(lo, hi, pen)
    if resident:
        return L.best_pair_by_offset(p, o, r_cat, r_off, c_off, st, ln, sd, cigar=cigar)
    return L.best_pair_windows(p, o, r_cat, r_off, target, c_off, st, ln, sd, cigar=cigar)


def _check(got, exp, cigar, what=""):
    assert got["best"].dtype == np.int32 and got["proper"].dtype == np.uint8 and got["tlen"].dtype == np.int64
    for key in ("cand_score", "cand_start", "cand_end", "best", "proper", "tlen", "second_score", "score", "target_start", "target_end"):
        assert got[key].shape == exp[key].shape, (what, key)
        assert np.array_equal(got[key], exp[key]), (what, key, np.flatnonzero(got[key] != exp[key])[:8], got[key][:12], exp[key][:12])
    if not cigar:
        assert got["ops"] is None and got["off"] is None
        return
    ops, off = got["ops"], got["off"]
    assert off.shape[0] == len(exp["routes"]) + 1 and off[0] == 0
    for r, route in enumerate(exp["routes"]):
        mine = [(int(x), int(o)) for x, o in zip(ops["run_length"][off[r]:off[r + 1]], ops["op"][off[r]:off[r + 1]])]
        assert mine == route, (what, "route of read", r, mine[:6], route[:6])


def _window_over(rng, target_len, pos, ln, wl):
    """a window of wl bases that covers [pos, pos + ln)"""
    s = pos - int(rng.integers(0, wl - ln + 1))
    return max(0, min(s, target_len - wl)), wl


KS = [(0, 3), (5, 5), (1, 1), (2, 4), (3, 0), (4, 2), (5, 1), (2, 2)]  # candidates of mate 1 / mate 2, pair by pair: 0 .. 5


def _workload(seed, sub=0.04, target_len=3000):
    """8 pairs: mates of 20 .. 40 bases from the two ends of a fragment of 150 .. 400 bases, the reverse one first in every other pair;
    candidate windows of 60 .. 160 bases, one over the mate's origin on the right strand (at a position that moves through the
    list), the others anywhere on either strand; a few N in the target"""
    rng = np.random.default_rng(seed)
    target = rng.integers(0, 4, size=target_len).astype(np.uint8)
    target[rng.integers(0, target_len, size=12)] = 4
    reads, cands = [], []
    for k, ks in enumerate(KS):
        frag, l1, l2 = int(rng.integers(150, 401)), int(rng.integers(20, 41)), int(rng.integers(20, 41))
        o = int(rng.integers(200, target_len - frag - 200))
        fwd = (common.mutate(rng, target[o:o + l1 + 5], sub=sub, indel=0.01)[:l1], o, l1, 0)
        rev = (_rc(common.mutate(rng, target[o + frag - l2 - 5:o + frag], sub=sub, indel=0.01)[-l2:]), o + frag - l2, l2, 1)
        for (rd, pos, ln, strand), K in zip((rev, fwd) if k % 2 else (fwd, rev), ks):
            reads.append(np.ascontiguousarray(rd, np.uint8))
            cs = []
            for x in range(K):
                wl = int(rng.integers(60, 161))
                if x == k % K:
                    cs.append(_window_over(rng, target_len, pos, ln, wl) + (strand,))
                else:
                    cs.append((int(rng.integers(0, target_len - wl)), wl, int(rng.integers(0, 2))))
            cands.append(cs)
    return reads, target, cands


LO, HI, PEN = 100, 500, 300


@functools.lru_cache(maxsize=None)
def _fuzz():
    reads, target, cands = _workload(2027)
    exp = _expected(MX["Default"], GO, GE, reads, target, cands, LO, HI, PEN)
    # what the case is for: proper and improper pairs, winners that are not the first candidate, both strand orders among the proper pairs
    assert 0 < int(exp["proper"].sum()) < len(KS) and any(b > 0 for b in exp["best"])
    first = [cands[2 * k][exp["best"][2 * k]][2] for k in range(len(KS)) if exp["proper"][k]]
    assert 0 in first and 1 in first
    assert sum(len(c) for c in cands) > 16  # (GNX_HOST_SUB=8: more than two sub-batches)
    return reads, target, cands, exp


def test_both_entries_on_both_strands(gpu_lib):
    """K = 0 .. 5 per mate, windows from a buffer and from the packed resident reference, with and without the CIGAR stage"""
    reads, target, cands, exp = _fuzz()
    p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
    for cigar in (True, False):
        _check(_call(gpu_lib, p, reads, target, cands, LO, HI, PEN, cigar=cigar), exp, cigar, "windows")
        tm = gpu_lib.get_timing()
        assert tm["fast_path"] == 10 and tm["n_contexts"] == 1, tm
        assert tm["cells"] == sum(len(r) * c[1] for r, cs in zip(reads, cands) for c in cs)
    gpu_lib.set_reference(target)
    try:
        for cigar in (True, False):
            _check(_call(gpu_lib, p, reads, None, cands, LO, HI, PEN, cigar=cigar, resident=True), exp, cigar, "resident")
            assert gpu_lib.get_timing()["fast_path"] == 10
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def test_sub_batches_straddle_a_pair(gpu_lib, monkeypatch):
    reads, target, cands, exp = _fuzz()
    p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
    monkeypatch.setenv("GNX_HOST_SUB", "8")
    c_off = exp["c_off"]
    assert any(c_off[2 * k] // 8 != (c_off[2 * k + 2] - 1) // 8 for k in range(len(KS)) if c_off[2 * k + 2] > c_off[2 * k])
    _check(_call(gpu_lib, p, reads, target, cands, LO, HI, PEN), exp, True, "GNX_HOST_SUB=8")
    assert gpu_lib.get_timing()["n_launches"] > 2
    gpu_lib.set_reference(target)
    try:
        _check(_call(gpu_lib, p, reads, None, cands, LO, HI, PEN, resident=True), exp, True, "GNX_HOST_SUB=8, resident")
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def test_fallback_routes(gpu_lib, monkeypatch):
    """GNX_SCORE_SWEEP=0 and gapOpen > 0: the score stage takes the align route and reads both positions off the CIGAR; the results
    stay what the oracle says"""
    reads, target, cands, exp = _fuzz()
    p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
    monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
    for cigar in (True, False):
        _check(_call(gpu_lib, p, reads, target, cands, LO, HI, PEN, cigar=cigar), exp, cigar, "GNX_SCORE_SWEEP=0")
        assert gpu_lib.get_timing()["fast_path"] not in (8, 10)
    gpu_lib.set_reference(target)
    try:
        _check(_call(gpu_lib, p, reads, None, cands, LO, HI, PEN, resident=True), exp, True, "GNX_SCORE_SWEEP=0, resident")
        assert gpu_lib.get_timing()["fast_path"] not in (8, 10)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    monkeypatch.delenv("GNX_SCORE_SWEEP")
    p = gpu_lib.make_params(LOCAL, MX["Default"], 25, GE)
    exp = _expected(MX["Default"], 25, GE, reads, target, cands, LO, HI, PEN)
    _check(_call(gpu_lib, p, reads, target, cands, LO, HI, PEN), exp, True, "gapOpen > 0")
    assert gpu_lib.get_timing()["fast_path"] not in (8, 10)


def _one_fragment(seed, ln, frag, wl, target_len=3000):
    """one pair from one fragment and a window of wl bases over each mate: (reads, target, (forward window, reverse window))"""
    rng = np.random.default_rng(seed)
    target = rng.integers(0, 4, size=target_len).astype(np.uint8)
    o = 1000
    reads = [common.mutate(rng, target[o:o + ln + 30], sub=0.03, indel=0.01)[:ln], _rc(common.mutate(rng, target[o + frag - ln - 30:o + frag], sub=0.03, indel=0.01)[-ln:])]
    return reads, target, ((o - (wl - ln) // 2, wl, 0), (o + frag - ln - (wl - ln) // 2, wl, 1))


def test_81_tied_combinations_go_to_the_first(gpu_lib):
    """9 x 9 candidates that are one window repeated: every combination is proper with the same score, spread over the lanes' strides;
    the winner is (0, 0) and the runner-up is the same score"""
    reads, target, (wf, wv) = _one_fragment(5, 30, 90, 160)
    w = (990, 160, 0)
    cands = [[w] * 9, [w[:2] + (1,)] * 9]
    exp = _expected(MX["Default"], GO, GE, reads, target, cands, 0, 1000, 0)
    assert all(pyref_pairs.insert(a, b, 0, 1000) is not None for a in exp["tables"][0] for b in exp["tables"][1])
    assert exp["best"].tolist() == [0, 0] and exp["proper"].tolist() == [1]
    got = _call(gpu_lib, gpu_lib.make_params(LOCAL, MX["Default"], GO, GE), reads, target, cands, 0, 1000, 0)
    _check(got, exp, True, "81 ties")
    assert got["best"].tolist() == [0, 0] and np.array_equal(got["second_score"], got["cand_score"][[0, 9]])


def test_only_the_last_of_81_combinations_is_proper(gpu_lib):
    """candidates 0 .. 7 of either mate are on the wrong strand, far out on the wrong side; 8 x 8 is the only proper combination, and a
    penalty larger than any score makes it win"""
    reads, target, (wf, wv) = _one_fragment(6, 30, 200, 120)
    cands = [[(100, 120, 1)] * 8 + [wf], [(2700, 120, 0)] * 8 + [wv]]
    exp = _expected(MX["Default"], GO, GE, reads, target, cands, 100, 400, 100000)
    n_proper = sum(pyref_pairs.insert(a, b, 100, 400) is not None for a in exp["tables"][0] for b in exp["tables"][1])
    assert n_proper == 1 and exp["best"].tolist() == [8, 8] and exp["proper"].tolist() == [1]
    _check(_call(gpu_lib, gpu_lib.make_params(LOCAL, MX["Default"], GO, GE), reads, target, cands, 100, 400, 100000), exp, True, "last of 81")


def test_reads_of_200_bases_take_the_hand_over_rows(gpu_lib):
    """queries of more than one 192-column strip of the span stage"""
    reads, target, (wf, wv) = _one_fragment(7, 200, 600, 400)
    assert len(reads[0]) == 200 and len(reads[1]) == 200
    cands = [[(50, 300, 1), wf], [wv, (2000, 350, 1), (1500, 250, 0)]]
    mx, (go, ge) = MX["HumanChimpTwo"], (-600, -150)
    exp = _expected(mx, go, ge, reads, target, cands, 300, 900, 0)
    assert exp["best"].tolist() == [1, 0] and exp["proper"].tolist() == [1]
    _check(_call(gpu_lib, gpu_lib.make_params(LOCAL, mx, go, ge), reads, target, cands, 300, 900, 0), exp, True, "200-base reads")
    assert gpu_lib.get_timing()["fast_path"] == 10


def test_unpaired_penalty_flips_the_decision(gpu_lib):
    """mate 2 has an exact copy far away that beats its clipped window next to mate 1: with penalty d = (sum of first maxima) - P the
    proper combination wins, with d - 1 it does not -- two calls that differ in nothing else"""
    reads, target, (wf, wv) = _one_fragment(8, 30, 200, 120)
    target = target.copy()
    target[2500:2530] = _rc(reads[1])
    clipped = (wv[0], 1170 + 24 - wv[0], 1)  # ends 6 bases short of the mate's end
    cands = [[wf], [(2460, 120, 1), clipped]]
    p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
    base = _expected(MX["Default"], GO, GE, reads, target, cands, 100, 400, 0)
    t1, t2 = base["tables"]
    assert pyref_pairs.insert(t1[0], t2[0], 100, 400) is None and pyref_pairs.insert(t1[0], t2[1], 100, 400) is not None
    d = t2[0][0] - t2[1][0]
    assert d > 1
    for pen, proper, best in ((d, 1, [0, 1]), (d - 1, 0, [0, 0])):
        exp = _expected(MX["Default"], GO, GE, reads, target, cands, 100, 400, pen)
        assert exp["proper"].tolist() == [proper] and exp["best"].tolist() == best
        _check(_call(gpu_lib, p, reads, target, cands, 100, 400, pen), exp, True, "penalty %d" % pen)


def test_a_bad_base_in_a_losing_candidate_fails_the_call(gpu_lib):
    reads, target, cands, _ = _fuzz()
    target = target.copy()
    target[2990] = 6
    bad = [list(cs) for cs in cands]
    bad[3].append((2989, 3, 0))  # three bases: it cannot win, and it touches the byte 6
    r_cat, r_off, c_off, st, ln, sd = _tables(reads, bad)
    st, ln, sd = np.asarray(st, np.int64), np.asarray(ln, np.int64), np.asarray(sd, np.uint8)
    n, nc = len(reads), len(st)
    p, o = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE), gpu_lib.pair_opts(LO, HI, PEN)
    best, per_read = np.full(n, 77, np.int32), [np.full(n, 77, np.int64) for _ in range(4)]
    proper, tlen, per_cand = np.full(n // 2, 77, np.uint8), np.full(n // 2, 77, np.int64), [np.full(nc, 77, np.int64) for _ in range(3)]
    ops, off = ctypes.c_void_p(), ctypes.c_void_p()
    rc = gpu_lib.lib().gnx_best_pair_windows(ctypes.byref(p), ctypes.byref(o), n, r_cat.ctypes.data, r_off.ctypes.data, target.ctypes.data, target.shape[0], c_off.ctypes.data,
                                             st.ctypes.data, ln.ctypes.data, sd.ctypes.data, best.ctypes.data, *[a.ctypes.data for a in per_read], proper.ctypes.data, tlen.ctypes.data,
                                             *[a.ctypes.data for a in per_cand], ctypes.byref(ops), ctypes.byref(off))
    assert rc == gpu_lib.GNX_EBASE
    assert all(np.all(a == 77) for a in [best, proper, tlen] + per_read + per_cand) and not ops.value and not off.value
    with pytest.raises(gpu_lib.GnxError) as ei:
        _call(gpu_lib, p, reads, target, bad, LO, HI, PEN, cigar=False)
    assert ei.value.code == gpu_lib.GNX_EBASE


def test_asymmetric_matrix(gpu_lib):
    """tests/asym.py's table: a transposed or complemented matrix anywhere in the score or span stage changes nearly every score"""
    reads, target, cands = _workload(2029, sub=0.12)
    go, ge = asym.AFFINE_PENS[0]
    ts, qs = _flatten(reads, target, cands)
    res = asym.assert_tells_orientation(LOCAL, go, ge, ts, qs, threads=16)
    asym.assert_tells_orientation(LOCAL, go, ge, ts, qs, other=asym.ASYM_RC, threads=16)
    exp = _expected(asym.ASYM, go, ge, reads, target, cands, LO, HI, PEN, res=res)
    assert int(exp["proper"].sum()) > 0
    p = gpu_lib.make_params(LOCAL, asym.ASYM, go, ge)
    _check(_call(gpu_lib, p, reads, target, cands, LO, HI, PEN), exp, True, "ASYM, windows")
    assert gpu_lib.get_timing()["fast_path"] == 10
    gpu_lib.set_reference(target)
    try:
        _check(_call(gpu_lib, p, reads, None, cands, LO, HI, PEN, resident=True), exp, True, "ASYM, resident")
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def test_degenerate_inputs(gpu_lib):
    p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
    reads, target, _, _ = _fuzz()
    for cigar in (True, False):
        got = _call(gpu_lib, p, reads[:4], target, [[], [], [], []], 0, 10, 0, cigar=cigar)
        assert got["best"].tolist() == [-1] * 4 and got["score"].tolist() == [0] * 4 and got["target_start"].tolist() == [0] * 4 and got["target_end"].tolist() == [0] * 4
        assert got["proper"].tolist() == [0, 0] and got["tlen"].tolist() == [0, 0] and got["second_score"].tolist() == [I64_MIN] * 4
        assert (got["off"].tolist() == [0] * 5 and got["ops"].shape == (0,)) if cigar else got["off"] is None
        got = _call(gpu_lib, p, [], target, [], 0, 10, 0, cigar=cigar)
        assert got["best"].shape == (0,) and got["proper"].shape == (0,) and (got["off"].tolist() == [0] if cigar else got["off"] is None)


def test_python_map_best_pair(gpu_lib):
    """align.MapBestPair with the windows taken from a given target and from the resident reference: the oracle's values per read"""
    reads, target, cands, exp = _fuzz()
    p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
    gpu_lib.set_reference(target)
    try:
        outs = [align.MapBestPair(p, reads, cands, LO, HI, PEN, target=target), align.MapBestPair(p, reads, cands, LO, HI, PEN)]
        bare = align.MapBestPair(p, reads, cands, LO, HI, PEN, cigar=False)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    want_pairs = [(bool(pr), int(t)) for pr, t in zip(exp["proper"], exp["tlen"])]
    for r, cs in enumerate(cands):
        b = int(exp["best"][r])
        ws = cs[b][0] if b >= 0 else None
        sec = int(exp["second_score"][r])
        want = (b, int(exp["score"][r]), [align.Cigar(x, o) for x, o in exp["routes"][r]], int(exp["target_end"][r]), [t[0] for t in exp["tables"][r]],
                ws + int(exp["target_start"][r]) if b >= 0 else None, ws + int(exp["target_end"][r]) if b >= 0 else None, None if sec == I64_MIN else sec)
        for per_read, per_pair in outs:
            assert per_read[r] == want, (r, per_read[r], want)
            assert per_pair == want_pairs
        assert bare[0][r] == want[:2] + (None,) + want[3:] and bare[1] == want_pairs


SYN_LEN, SYN_SEED, K = 65536, 11, 16


@functools.lru_cache(maxsize=None)
def _simulated_pairs():
    """36 pairs of 100-base mates with 0 .. 3 substitutions from fragments of 250 .. 450 bases of the synthetic reference, the reverse
    mate first in every other pair"""
    rng = np.random.default_rng(41)
    ref = _lib.synthetic_reference_bases(0, SYN_LEN, SYN_SEED)
    reads = []
    for k in range(36):
        frag = int(rng.integers(250, 451))
        o = int(rng.integers(0, SYN_LEN - frag))
        pieces = [ref[o:o + 100].copy(), ref[o + frag - 100:o + frag].copy()]
        for x in pieces:
            for at in rng.choice(100, size=int(rng.integers(0, 4)), replace=False):
                x[at] = (x[at] + rng.integers(1, 4)) % 4
        mates = [pieces[0], _rc(pieces[1])]
        reads += mates[::-1] if k % 2 else mates
    return reads


def test_map_read_pairs_equals_seed_candidates_then_map_best_pair(gpu_lib):
    reads = _simulated_pairs()
    gpu_lib.check(gpu_lib.lib().gnx_set_reference_synthetic(SYN_LEN, SYN_SEED))
    try:
        gpu_lib.reference_index_build(K, 1)
        p = gpu_lib.make_params(LOCAL, MX["Default"], GO, GE)
        vote = dict(max_occ=16, bin=32, pad=16, max_cand=4, min_votes=2)
        got = align.MapReadPairs(p, reads, 150, 600, 200, **vote)
        voted = align.SeedCandidates(reads, **vote)
        exp = align.MapBestPair(p, reads, [[c[:3] for c in cs] for cs in voted], 150, 600, 200)
        assert got == exp
        per_read, per_pair = got
        assert len(per_read) == 72 and len(per_pair) == 36
        assert sum(pr for pr, _ in per_pair) >= 18  # (a condition on the inputs: the span checks below run for most of the pairs)
        for k, (proper, tlen) in enumerate(per_pair):
            if not proper:
                assert tlen == 0
                continue
            spans = []
            for r in (2 * k, 2 * k + 1):
                best, score, route, t_end, cand_scores, a_start, a_end, second = per_read[r]
                w_start, w_len, strand, _ = voted[r][best]
                lead = route[0].RunLength if len(route) > 1 and route[0].Op == COL_D else 0
                trail = route[-1].RunLength if route[-1].Op == COL_D else 0
                assert (a_start, a_end, t_end) == (w_start + lead, w_start + w_len - trail, w_len - trail), (k, r)
                assert score == cand_scores[best] and (second is None) == (len(cand_scores) == 1)
                spans.append((a_start, a_end, strand))
            f, v = sorted(spans, key=lambda s: s[2])
            assert f[2] == 0 and v[2] == 1 and tlen == v[1] - f[0] and 150 <= tlen <= 600
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
