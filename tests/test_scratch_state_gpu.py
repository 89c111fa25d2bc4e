"""No result may depend on what a call finds in its workspace.

The library keeps one context per device for the life of the process: about 176 device buffers and nine pinned ones that only grow and
that nothing clears between calls.  A route is correct only while it initialises every word it reads before it writes it, and the other
suites run each route once, on buffers that are fresh (cleared by the driver) or left by whichever test ran before.  Here

(a) every route runs, the whole workspace is then filled with a pattern (gnx_debug_fill_scratch: scratch buffers whole, state buffers
    behind what their owner wrote, the cached plans dropped), and the route runs again: the second result is the reference's -- under
    four patterns that disagree with each other (zeroes; all ones: claim, progress and flag words; 0x80808080: the "not written yet"
    of the hand-over rows; 0x3F3F3F3F: a large score that wins every max without overflowing).  For the routes with state -- the
    resident reference, its index, the seed index, the pile and its log -- the pattern comes between the call that sets the state and
    the call that reads it, and between two adds;
(b) every align route runs big, small, big' with nothing in between: a real predecessor's plausible values behind the small batch's
    extent, and one chain across the routes that share trace, hcol, rowbuf, dcol and plans;
(c) the fast path's device-resident plan cache: equal lengths with other bases must hit, one window one base longer must miss
    (gnx_debug_counter(12 / 13)), and every result is the oracle's.

Every comparison is exact; batches, references and route switches are those of tests/test_asym_gpu.py and of the suites of each
entry point.  Each case asserts the route it ran on in BOTH runs.  Sensitivity rests on the four patterns disagreeing, not on a run of
a broken build."""
import collections
import functools

import numpy as np
import pytest

import asym
import common
import oracle
from asym import ASYM

pytestmark = pytest.mark.gpu

PATTERNS = (0x00000000, 0xFFFFFFFF, 0x80808080, 0x3F3F3F3F)
ROUTE_SWITCHES = ("GNX_FASTPATH", "GNX_NO_HFORM", "GNX_LAT", "GNX_WIDE", "GNX_CLONG", "GNX_W64", "GNX_REBASE", "GNX_CL_CKC", "GNX_MEGA_STRIPS",
                  "GNX_W64_FARM", "GNX_W64_SPEC", "GNX_W64_FARM_PIPE", "GNX_W64_CK", "GNX_FP_MAXIT", "GNX_TB_TWO_PASS", "GNX_SCORE_SWEEP", "GNX_NO_PIPE",
                  "GNX_FP_CERT", "GNX_SEED_VOTE_LDS", "GNX_SEED_SUB", "GNX_SUMMARY_FORM", "GNX_SUMMARY_SUB", "GNX_MD_FORM", "GNX_MD_SUB", "GNX_PILE_FORM",
                  "GNX_PILE_SUB", "GNX_NORM_COOP", "GNX_SCORED_SUB")

Case = collections.namedtuple("Case", "env run align")  # run(L, dirty): one run of the case, asserting result AND route; align: (batch, mode, go, ge, ci, route) or None
ROUTES = collections.OrderedDict()


@pytest.fixture(autouse=True)
def _own_switches(monkeypatch):
    for k in ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


def _route_is(tm, route, what):
    if route in (0, 1, 2):
        common.expect_route(tm, route)
    elif not common.OUTER_ROUTE_SWITCH:
        assert tm["fast_path"] == route, (tm["fast_path"], route, what)


def _no_reference(L):
    L.set_reference(np.zeros(0, np.uint8))


# ---- the align routes --------------------------------------------------------------------------------------------------------------------
def _floor(name):
    """the fewest rows a read of this batch may have and stay on its route (the fast path's row blocks)"""
    return 160 * (int(name[2]) - 1) + 1 if name[:2] in ("fp", "xp") and name[2:].isdigit() else 1


@functools.lru_cache(maxsize=None)
def variant(name, which):
    """big: the named batch of tests/asym.py.  other: the same lengths with other bases -- every sequence reversed (a read stays related
    to its window).  small: the first half of the pairs, every sequence cut (reads by a quarter, down to their route's floor; everything
    else by a third): strictly fewer pairs, a strictly shorter longest row and column."""
    alphas, betas = asym.batch(name)
    if which == "big":
        return alphas, betas
    if which == "other":
        return [np.ascontiguousarray(a[::-1]) for a in alphas], [np.ascontiguousarray(b[::-1]) for b in betas]
    half = max(1, len(alphas) // 2)
    lo = _floor(name)
    reads_are_beta = name.startswith("xp")

    def cut(x, is_read):
        keep = max(lo, len(x) - max(1, len(x) // 4)) if (is_read and lo > 1) else max(1, len(x) - max(1, len(x) // 3))
        return np.ascontiguousarray(x[:min(keep, len(x))])
    sa = [cut(a, not reads_are_beta) for a in alphas[:half]]
    sb = [cut(b, reads_are_beta) for b in betas[:half]]
    assert len(sa) < len(alphas)
    # (the longest row may stay where a read already sits on its route's floor -- one base fewer and a fast-path batch of S row blocks would
    # be one of S - 1, another route; everywhere else rows and columns are strictly shorter)
    assert max(map(len, sb if reads_are_beta else sa)) < max(map(len, betas if reads_are_beta else alphas)) or lo > 1
    assert max(map(len, sa)) <= max(map(len, alphas)) and max(map(len, sb)) <= max(map(len, betas))
    assert max(map(len, sa if reads_are_beta else sb)) < max(map(len, alphas if reads_are_beta else betas))
    return sa, sb


@functools.lru_cache(maxsize=None)
def expected(name, which, mode, go, ge, ci):
    if which == "big":
        return asym.expected(name, mode, "ASYM", go, ge, ci)
    alphas, betas = variant(name, which)
    return oracle.align_batch(mode, ASYM, go, ge, alphas, betas, ci, ci, threads=8)


def _align_once(L, name, which, mode, go, ge, ci, route, what):
    alphas, betas = variant(name, which)
    got = L.align_batch(L.make_params(mode, ASYM, go, ge, ci, ci), alphas, betas)
    tm = L.get_timing()
    common.assert_same(got, expected(name, which, mode, go, ge, ci), "%s/%s mode %d (%d, %d) checkersize %d %s" % (name, which, mode, go, ge, ci, what))
    _route_is(tm, route, (name, which, mode, what))


def _align_case(key, env, name, mode, route, ci=10000, pen=None):
    go, ge = pen or asym.pens(mode)[-1]
    assert key not in ROUTES
    ROUTES[key] = Case(env, lambda L, dirty: _align_once(L, name, "big", mode, go, ge, ci, route, key), (name, mode, go, ge, ci, route))


GENERAL = {"GNX_FASTPATH": "0"}
for _m in range(5):
    for _b in ("small", "long16"):
        _align_case("stored_hform/%s/mode%d" % (_b, _m), GENERAL, _b, _m, 0)
        _align_case("stored_plain/%s/mode%d" % (_b, _m), dict(GENERAL, GNX_NO_HFORM="1"), _b, _m, 0)
    _align_case("coop_traceback/mode%d" % _m, GENERAL, "coop", _m, 0)
    _align_case("two_pass_traceback/mode%d" % _m, dict(GENERAL, GNX_TB_TWO_PASS="1"), "coop", _m, 0)
    for _b in ("small", "tall12"):
        _align_case("latency/%s/mode%d" % (_b, _m), {"GNX_LAT": "2"}, _b, _m, 3)
    for _b in ("small", "long16"):
        _align_case("int64/%s/mode%d" % (_b, _m), {"GNX_WIDE": "2"}, _b, _m, 4)
for _lm in (0, 1):
    _align_case("stored_hform/small/mode%d/checker7" % _lm, GENERAL, "small", _lm, 0, ci=7)
for _k in (1, 2, 3):
    _align_case("fast_path/%d_blocks/global" % _k, {"GNX_FASTPATH": "2"}, "fp%d" % _k, 0, 1)
    _align_case("fast_path/%d_blocks/transposed" % _k, {"GNX_FASTPATH": "2"}, "xp%d" % _k, 3, 1)
_align_case("fast_path/overflow_redo/global", {"GNX_FASTPATH": "2"}, "fp_cheap", 0, 1, pen=asym.CHEAP_GAPS)
_align_case("fast_path/overflow_redo/transposed", {"GNX_FASTPATH": "2"}, "xp_cheap", 3, 1, pen=asym.CHEAP_GAPS)
for _m, _cs in [(0, 3), (0, 10000), (1, 3), (1, 10000), (2, 10000), (4, 10000)]:
    for _rb in (False, True):
        _env = {"GNX_CLONG": "2", "GNX_W64": "0"}
        if _rb:
            _env["GNX_REBASE"] = "1"
        _align_case("snapshot16/%s/mode%d/checker%d" % ("rebase" if _rb else "static", _m, _cs), _env, "long40", _m, 2, ci=_cs)
for _m, _cs in [(0, 16), (0, 10000), (1, 16), (1, 10000), (2, 10000), (4, 10000)]:
    for _walk, _env in (("farm", {}), ("two_waves", {"GNX_W64_FARM": "0"}), ("one_wave", {"GNX_W64_FARM": "0", "GNX_W64_SPEC": "0"})):
        _align_case("snapshot64/%s/mode%d/checker%d" % (_walk, _m, _cs), dict(_env, GNX_CLONG="2", GNX_W64="2"), "w64", _m, 6, ci=_cs)
for _m in (0, 1):
    _align_case("snapshot64/rebase/mode%d" % _m, {"GNX_CLONG": "2", "GNX_W64": "2", "GNX_REBASE": "1"}, "w64", _m, 6)
for _m in (0, 1, 2, 4):
    _align_case("row_panels16/mode%d" % _m, {"GNX_MEGA_STRIPS": "2"}, "panels", _m, 5)
    _align_case("row_panels64/mode%d" % _m, {"GNX_MEGA_STRIPS": "2", "GNX_W64": "2"}, "panels", _m, 5)
ALIGN_KEYS = [k for k, c in ROUTES.items() if c.align]


# ---- the gapless certificate forced on ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cert_batch():
    import test_fp_cert_gpu as tfc
    from gonomics_amd import _lib
    reads, wins, exp, meta = tfc.batch(4124, 24, kinds=tfc.SURE + ("indel",), ms=(300, 2000), ns=tfc.N_CERTIFIABLE)  # 18 certified, 6 with an indel live
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, tfc.HCT, tfc.GO, tfc.GE)
    host = sum(1 for a, b in zip(reads, wins) if _lib.debug_gapless_certificate(p, a, b, K=16)[0])
    return reads, wins, exp, host


def _certificate(L, dirty):
    import test_fp_cert_gpu as tfc
    reads, wins, exp, host = _cert_batch()
    assert 0 < host < len(reads)  # (a live list that is neither empty nor everything)
    L.debug_counter(9); L.debug_counter(10); L.debug_counter(11)
    got = L.align_batch(L.make_params(L.GNX_AFFINE_GAP, tfc.HCT, tfc.GO, tfc.GE), list(reads), list(wins))
    assert L.get_timing()["fast_path"] == 1
    common.assert_same(got, exp, "gapless certificate forced on")
    assert (L.debug_counter(9) + L.debug_counter(11), L.debug_counter(10)) == (host, len(reads))  # a stale flag would certify other pairs


ROUTES["fast_path/certificate_forced"] = Case({"GNX_FASTPATH": "2", "GNX_FP_CERT": "2"}, _certificate, None)


# ---- the score sweep, locate and span ------------------------------------------------------------------------------------------------------
def _score_sweep(mode):
    go, ge = asym.pens(mode)[-1]

    def run(L, dirty):
        alphas, betas = asym.batch("sweep")
        got = L.score_batch(L.make_params(mode, ASYM, go, ge), alphas, betas)
        assert L.get_timing()["fast_path"] == 7
        exp = np.asarray(asym.expected("sweep", mode, "ASYM", go, ge)[0], dtype=np.int64)
        assert np.array_equal(got, exp), (mode, np.flatnonzero(got != exp)[:8])
    return run


@functools.lru_cache(maxsize=None)
def _by_offset_expected(mode, go, ge):
    ref, reads, w_start, w_len = asym.global_ref_batch()
    return oracle.align_batch(mode, ASYM, go, ge, reads, [ref[s:s + l] for s, l in zip(w_start, w_len)], threads=8)


def _score_sweep_by_offset(mode):
    go, ge = asym.pens(mode)[-1]

    def run(L, dirty):
        ref, reads, w_start, w_len = asym.global_ref_batch()
        cat = np.concatenate(reads)
        off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
        exp = _by_offset_expected(mode, go, ge)
        L.set_reference(ref)
        try:
            dirty()  # the packed reference stands; its slack and every scratch buffer are dirt
            p = L.make_params(mode, ASYM, go, ge)
            got = L.score_batch_by_offset(p, cat, off, w_start, w_len)
            assert L.get_timing()["fast_path"] == 7
            assert np.array_equal(got, exp[0]), np.flatnonzero(got != exp[0])[:8]
            dirty()
            common.assert_same(L.align_batch_by_offset(p, cat, off, w_start, w_len), exp, "align twin by offset, mode %d" % mode)
        finally:
            _no_reference(L)
    return run


for _m in (0, 1, 2, 4):
    ROUTES["score_sweep/mode%d" % _m] = Case({}, _score_sweep(_m), None)
    ROUTES["score_sweep_by_offset/mode%d" % _m] = Case({}, _score_sweep_by_offset(_m), None)


@functools.lru_cache(maxsize=None)
def _local_spans():
    import pyref_span
    targets, queries = asym.batch("local")
    return pyref_span.spans_from_oracle(ASYM, -600, -150, targets, queries, threads=8)


def _locate(span):
    def run(L, dirty):
        targets, queries = asym.batch("local")
        ref, t_start, t_len, queries2 = asym.local_ref_batch()
        q_cat = np.concatenate(queries)
        q_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
        S, start, end = _local_spans()
        p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, ASYM, -600, -150)
        L.set_reference(ref)
        try:
            if span:
                calls = [("locate_span_batch", lambda: L.locate_span_batch(p, targets, queries)),
                         ("locate_span_batch_by_offset", lambda: L.locate_span_batch_by_offset(p, q_cat, q_off, t_start, t_len))]
            else:
                calls = [("locate_batch", lambda: L.locate_batch(p, targets, queries)),
                         ("locate_batch_windows", lambda: L.locate_batch_windows(p, ref, t_start, t_len, q_cat, q_off[:-1], np.diff(q_off))),
                         ("locate_batch_by_offset", lambda: L.locate_batch_by_offset(p, q_cat, q_off, t_start, t_len))]
            for what, fn in calls:
                dirty()
                out = fn()
                assert L.get_timing()["fast_path"] == (10 if span else 8), (what, L.get_timing()["fast_path"])
                assert np.array_equal(out[0], S), (what, "score", np.flatnonzero(out[0] != S)[:8])
                assert np.array_equal(out[-1], end), (what, "end", np.flatnonzero(out[-1] != end)[:8])
                if span:
                    assert np.array_equal(out[1], start), (what, "start", np.flatnonzero(out[1] != start)[:8])
        finally:
            _no_reference(L)
    return run


ROUTES["locate"] = Case({}, _locate(False), None)
ROUTES["locate_span"] = Case({}, _locate(True), None)


# ---- AffineGapChunk and the multiple alignment by each of their routes --------------------------------------------------------------------
def _n1_got(sc, ops, off, k):
    return (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])


@functools.lru_cache(maxsize=None)
def _chunk_expected(chunk):
    alphas, betas = asym.chunk_pairs(chunk)
    return [oracle.affine_gap_chunk(ASYM, -600, -150, chunk, a, b) for a, b in zip(alphas, betas)]


def _chunk(chunk, how):
    def run(L, dirty):
        alphas, betas = asym.chunk_pairs(chunk)
        exp = _chunk_expected(chunk)
        p = L.make_params(L.GNX_AFFINE_GAP_HIGHMEM, ASYM, -600, -150)
        sc, ops, off = L.affine_gap_chunk_batch(p, chunk, alphas, betas)
        twin = L.get_timing()["fast_path"]
        if not common.OUTER_ROUTE_SWITCH:
            assert twin == N1_ROUTE[how], (how, twin)
        for k in range(len(alphas)):
            assert _n1_got(sc, ops, off, k) == exp[k], (chunk, how, k)
        dirty()
        got = L.affine_gap_chunk_score_batch(p, chunk, alphas, betas)
        route = L.get_timing()["fast_path"]
        assert [int(x) for x in got] == [e[0] for e in exp], (chunk, how)
        if not common.OUTER_ROUTE_SWITCH:
            assert (route == 9) if how != "int64" else (route == 4), (how, route)
    return run


@functools.lru_cache(maxsize=None)
def _multi_expected(chunk):
    blocks, pairs = asym.groups(chunk)
    return [oracle.multiple_affine_gap(ASYM, -600, -150, chunk, blocks[x], blocks[y]) for x, y in pairs]


def _multi(chunk, how):
    def run(L, dirty):
        blocks, pairs = asym.groups(chunk)
        exp = _multi_expected(chunk)
        p = L.make_params(L.GNX_AFFINE_GAP_HIGHMEM, ASYM, -600, -150)
        sc, ops, off = L.multiple_affine_gap_batch(p, chunk, blocks, pairs)
        twin = L.get_timing()["fast_path"]
        if not common.OUTER_ROUTE_SWITCH:
            assert twin == N1_ROUTE[how], (how, twin)
        for k in range(len(pairs)):
            assert _n1_got(sc, ops, off, k) == exp[k], (chunk, pairs[k])
        dirty()
        got = L.multiple_affine_gap_score_batch(p, chunk, blocks, pairs)
        assert common.OUTER_ROUTE_SWITCH or L.get_timing()["fast_path"] == (4 if how == "int64" else 9)
        assert [int(x) for x in got] == [e[0] for e in exp], chunk
    return run


N1_ROUTE = {"lat": 3, "general": 0, "int64": 4}  # the align entries: latency geometry (the shipped routing of a small batch), stored matrix, int64 kernel
N1_ENV = {"lat": {"GNX_FP_SMALL": None}, "general": {"GNX_LAT": "0"}, "int64": {"GNX_WIDE": "2"}}
for _c in (1, 5):
    for _how in ("lat", "general", "int64"):
        ROUTES["affine_gap_chunk/%s/chunk%d" % (_how, _c)] = Case(N1_ENV[_how], _chunk(_c, _how), None)
for _c in (1, 2):
    for _how in ("lat", "general", "int64"):
        ROUTES["multiple_affine_gap/%s/chunk%d" % (_how, _c)] = Case(N1_ENV[_how], _multi(_c, _how), None)


# ---- best of K, best pair, seed candidates -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _best_of_expected(mode, go, ge):
    import test_best_of_gpu as bo
    reads, target, cands = asym.best_of_workload()
    return bo._expected(mode, ASYM, go, ge, reads, target, cands, 10000, 10000)


def _best_of(mode):
    go, ge = asym.pens(mode)[-1]

    def run(L, dirty):
        import test_best_of_gpu as bo
        reads, target, cands = asym.best_of_workload()
        exp = _best_of_expected(mode, go, ge)
        p = L.make_params(mode, ASYM, go, ge)
        bo._check(bo._call(L, p, reads, target, cands, cigar=True), exp, mode, True, "best_of_windows")
        L.set_reference(target)
        try:
            dirty()
            bo._check(bo._call(L, p, reads, None, cands, cigar=True, resident=True), exp, mode, True, "best_of_by_offset")
            dirty()
            bo._check(bo._call(L, p, reads, None, cands, cigar=False, resident=True), exp, mode, False, "best_of_by_offset, no CIGAR stage")
            assert L.get_timing()["fast_path"] == (8 if mode == 3 else 7)
        finally:
            _no_reference(L)
    return run


for _m in (0, 1, 3):
    ROUTES["best_of/mode%d" % _m] = Case({}, _best_of(_m), None)


@functools.lru_cache(maxsize=None)
def _best_pair_case():
    import test_best_pair_gpu as bp
    reads, target, cands = bp._workload(2029, sub=0.12)
    go, ge = asym.AFFINE_PENS[0]
    return reads, target, cands, go, ge, bp._expected(ASYM, go, ge, reads, target, cands, bp.LO, bp.HI, bp.PEN)


def _best_pair(L, dirty):
    import test_best_pair_gpu as bp
    reads, target, cands, go, ge, exp = _best_pair_case()
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, ASYM, go, ge)
    bp._check(bp._call(L, p, reads, target, cands, bp.LO, bp.HI, bp.PEN), exp, True, "best pair, windows")
    assert L.get_timing()["fast_path"] == 10
    L.set_reference(target)
    try:
        dirty()
        bp._check(bp._call(L, p, reads, None, cands, bp.LO, bp.HI, bp.PEN, resident=True), exp, True, "best pair, resident")
        assert L.get_timing()["fast_path"] == 10
    finally:
        _no_reference(L)


ROUTES["best_pair"] = Case({}, _best_pair, None)


def _seed_candidates(L, dirty):
    import test_ref_seeds_gpu as trs
    trs._STATE[0] = None  # (that module's note of what it left resident)
    exp, opts = trs._suite_expected("min_votes_1", 1)
    L.set_reference(trs.fixture_ref())
    try:
        dirty()
        L.reference_index_build(trs.K, 1)
        dirty()  # reference and index stand
        trs._same(trs._run(L, trs.suite_reads(), opts), exp, "seed candidates")
        assert L.get_timing()["fast_path"] == 11
        dirty()
        keys, pos = L.reference_index_get()
        table = _seed_index()
        assert keys.tolist() == [c for c, _ in table] and pos.tolist() == [q for _, q in table]
    finally:
        _no_reference(L)


@functools.lru_cache(maxsize=None)
def _seed_index():
    import pyref_seeds
    import test_ref_seeds_gpu as trs
    return pyref_seeds.index(trs.fixture_ref(), trs.K, 1)


ROUTES["seed_candidates/lds"] = Case({}, _seed_candidates, None)
ROUTES["seed_candidates/slab"] = Case({"GNX_SEED_VOTE_LDS": "0"}, _seed_candidates, None)


# ---- the graph aligner -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gsw_expected(side):
    pairs = asym.gsw_pairs(side)
    return [oracle.gsw_extend(side, ASYM, asym.GSW_GAP, a, b) for a, b in pairs]


def _gsw_extend(side):
    def run(L, dirty):
        from gonomics_amd import cigar, genomeGraph
        pairs = asym.gsw_pairs(side)
        got = genomeGraph.DynamicAlnBatch("left" if side == 0 else "right", [a for a, _ in pairs], [b for _, b in pairs], ASYM, asym.GSW_GAP)
        for k, ((score, route, i, j), (es, er, ei, ej)) in enumerate(zip(got, _gsw_expected(side))):
            assert (score, i, j) == (es, ei, ej), (side, k)
            assert [(c.RunLength, c.Op) for c in route] == [(r, cigar.from_col(o)) for r, o in er], (side, k)
    return run


# (the graph aligner's entries -- gsw_extend, the seed search, map-reads -- have one route each and leave no route in the timing that any suite
# reads: tests/test_n2_gsw.py, test_gsw_reads.py and test_seed_adversarial.py assert none either.  Their cases assert results only.)
ROUTES["gsw_extend/left"] = Case({}, _gsw_extend(0), None)
ROUTES["gsw_extend/right"] = Case({}, _gsw_extend(1), None)


@functools.lru_cache(maxsize=None)
def _gsw_reads_case(kind):
    import pyref_gsw as ref
    import test_gsw_reads as tg
    seqs, edges, reads = tg.make_case(17, kind)
    nodes = ref.make_graph(seqs, edges)
    full = ref.index_genome(nodes, 16, 1)
    keys = []
    for rd in reads:
        r2 = ref.make_read(rd)
        keys.append(ref.giraf_key(ref.read_to_giraf(nodes, r2, ref.seed_map(full, nodes, r2, 16), ASYM)))
    return seqs, edges, reads, keys


def _gsw_map_reads(kind):
    def run(L, dirty):
        import test_gsw_reads as tg
        from gonomics_amd import genomeGraph as gg
        seqs, edges, reads, keys = _gsw_reads_case(kind)
        bigs = [gg.FastqBig("r%d" % k, rd) for k, rd in enumerate(reads)]
        ng = gg.NativeGraph(tg.build(seqs, edges), 16, 1)  # (builds the index on the device, which leaves NO index resident)
        try:
            for again in (False, True):
                if again:
                    dirty()  # the first batch set the handle's seed index; it stands, and the second batch searches it without a new upload
                got = ng.GswBatchToGiraf([gg.FastqBig(b.Name, b.Seq.copy()) for b in bigs], ASYM, on_panic="mark")
                for k in range(len(reads)):
                    assert not isinstance(got[k], gg.GoPanic) and got[k].key() == keys[k], ("read %d" % k, again)
        finally:
            ng.handle.close()
    return run


@functools.lru_cache(maxsize=None)
def _seed_find_case():
    import gsw_adversarial as adv
    import test_seed_adversarial as tsa
    g = tsa.graph()
    return g, adv.case()[2], adv.ref_raw_hits(16, 1)


def _seed_index_find(L, dirty):
    """gnx_seed_index_set_gen, then gnx_seed_find_batch_gen twice against the index as it stands: L.seed_find_batch uploads only when other
    arrays come in, and the generation it holds shows that the second and third search ran on the first call's upload"""
    from gonomics_amd import genomeGraph as gg
    g, reads, exp = _seed_find_case()
    index = gg.SeedIndex(g.Nodes, 16, 1)  # (gnx_seed_index_build: no index is resident afterwards)
    node_seqs = [n.Seq for n in g.Nodes]
    dirty()
    assert L.seed_find_batch(index.keys, index.locs, node_seqs, reads, 16) == exp
    gen = L._seed_set[0][4]
    dirty()  # keys, locations, node words and offsets stand; their slack and every scratch buffer are dirt
    assert L.seed_find_batch(index.keys, index.locs, node_seqs, reads, 16) == exp
    dirty()
    assert L.seed_find_batch(index.keys, index.locs, node_seqs, reads[::-1], 16)[::-1] == exp
    assert L._seed_set[0][4] == gen and gen != 0, "the index was uploaded again: the searches did not run on the dirtied one"


ROUTES["seed_index_set_and_find"] = Case({}, _seed_index_find, None)


ROUTES["gsw_map_reads/linear"] = Case({}, _gsw_map_reads("linear"), None)
ROUTES["gsw_map_reads/wide"] = Case({}, _gsw_map_reads("wide"), None)


# ---- summaries, the extended CIGAR and MD in both walking forms ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _summary_expected(mode):
    import pyref_summary as ref
    import summary_cases as sc
    _, mx, go0, ge0 = sc.SCORING[0]
    go, ge = sc.pens(mode, go0, ge0)
    return [ref.summarize(mode, mx, go, ge, c[1], c[2], c[3]) for c in sc.seam_cases()]


def _summary(mode):
    def run(L, dirty):
        import pyref_summary as ref
        import summary_cases as sc
        import test_summary_gpu as tsg
        from gonomics_amd import align
        cases = sc.seam_cases()
        _, mx, go0, ge0 = sc.SCORING[0]
        go, ge = sc.pens(mode, go0, ge0)
        routes = [c[3] for c in cases]
        ops, off = align._routes_to_ops(routes)
        out, xops, xoff = L.summarize_batch(L.make_params(mode, mx, go, ge), [c[1] for c in cases], [c[2] for c in cases], ops, off, xcigar=True)
        t = L.get_timing()
        assert t["fast_path"] == 12 and t["cells"] == sum(r for route in routes for r, _ in route)
        for k, (exp, ex) in enumerate(_summary_expected(mode)):
            assert {f: int(out[f][k]) for f in ref.FIELDS} == exp and int(out["_reserved"][k]) == 0, (mode, cases[k][0])
            assert tsg._route(xops[xoff[k]:xoff[k + 1]]) == ex, (mode, cases[k][0])
    return run


@functools.lru_cache(maxsize=None)
def _md_expected(mode):
    import pyref_md as ref
    import summary_cases as sc
    return [ref.md(mode, c[1], c[2], c[3]) for c in sc.seam_cases()]


def _md(mode):
    def run(L, dirty):
        import summary_cases as sc
        import test_md_gpu as tmd
        cases = sc.seam_cases()
        routes = [c[3] for c in cases]
        got = tmd._device_md(tmd._params(mode), [c[1] for c in cases], [c[2] for c in cases], routes)
        t = L.get_timing()
        assert t["fast_path"] == 13 and t["cells"] == sum(r for route in routes for r, _ in route)
        want = _md_expected(mode)
        wrong = [(cases[k][0], got[k][:60], want[k][:60]) for k in range(len(cases)) if got[k] != want[k]]
        assert not wrong, (mode, wrong)
    return run


for _m in range(5):
    for _form in ("0", "1"):
        ROUTES["summary_xcigar/form%s/mode%d" % (_form, _m)] = Case({"GNX_SUMMARY_FORM": _form}, _summary(_m), None)
        ROUTES["md/form%s/mode%d" % (_form, _m)] = Case({"GNX_MD_FORM": _form}, _md(_m), None)


# ---- the pile: the pattern between adds, and between an add and a query --------------------------------------------------------------------
def _halves(batch, quals=None):
    """a pile batch in two adds (counts and events add up to the whole batch's)"""
    h = len(batch[0]) // 2
    a, b = tuple(x[:h] for x in batch), tuple(x[h:] for x in batch)
    return [(a, quals[:h] if quals is not None else None), (b, quals[h:] if quals is not None else None)]


def _pile_genome(L):
    import test_summary_gpu as tsg
    g, _ = tsg._resident_cases()
    L.set_reference(g)
    return g


def _pile_plain(L, dirty):
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    names, batch, want = tpg._seams()
    g = _pile_genome(L)
    try:
        dirty()
        align.PileupOpen(0, len(g))
        for part, _ in _halves(batch):
            dirty()  # between the open and an add, and between two adds: the counters stand
            tpg._add(tpg._params(), part)
            assert L.get_timing()["fast_path"] == 14
        dirty()
        got = align.PileupGet()
        assert not tpg._differences(got, want, 0), tpg._differences(got, want, 0)
        assert align.PileupInfo()["reads_added"] == len(names)
    finally:
        _no_reference(L)


@functools.lru_cache(maxsize=None)
def _pile_calls_case():
    import pileup_cases as pc
    import pyref_pileup as ref
    import test_summary_gpu as tsg
    g, _ = tsg._resident_cases()
    batch = pc.call_batch(g)
    start, n = pc.CALL_REGION
    pile = pc.restate(g, pc.CALL_REGION, *batch)
    return batch, pile, ref.calls(pile, g[start:start + n], pc.CALL_OPTS, region_start=start)


def _pile_calls(L, dirty):
    import pileup_cases as pc
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    batch, pile, want = _pile_calls_case()
    _pile_genome(L)
    try:
        start, n = pc.CALL_REGION
        align.PileupOpen(start, n)
        tpg._add(tpg._params(), batch)
        dirty()  # between the add and the query
        o = pc.CALL_OPTS
        got = L.pileup_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"])
        assert tpg._call_tuples(got) == want and (got["_pad"] == 0).all()
        t = L.get_timing()
        assert t["fast_path"] == 15 and t["cells"] == n
        assert (align.PileupGet() == tpg._as_rows(pile)).all()
    finally:
        _no_reference(L)


def _pile_alleles(L, dirty):
    import pyref_pile_alleles as ref
    import test_pile_alleles_gpu as tpa
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    names, batch, rows, alleles = tpa._seams()
    want = ref.listed(alleles)
    g = _pile_genome(L)
    try:
        tpa._open_tracking(0, len(g))
        events = 0
        for part, _ in _halves(batch):
            dirty()  # the slack of the log is dirt while the first add's events stand in it
            tpg._add(tpg._params(), part)
            assert L.get_timing()["fast_path"] == 14
            assert align.PileupAlleleInfo()["events"] >= events
            events = align.PileupAlleleInfo()["events"]
        assert events == 2 * len(want)
        dirty()
        assert tpa._allele_tuples(L.pileup_alleles()) == want
        t = L.get_timing()
        assert t["fast_path"] == 16 and t["cells"] == 2 * len(want)
        dirty()
        assert (align.PileupGet() == rows).all()
        assert tpa._allele_tuples(L.pileup_alleles()) == want  # (a query leaves the log as it was)
    finally:
        _no_reference(L)


@functools.lru_cache(maxsize=None)
def _pile_norm_case():
    import pileup_cases as pc
    import test_pile_norm_gpu as tpn
    g, b, planted, ins_want = tpn._seam_case()
    return g, b.all(), pc.opts(), tpn._restated(g, (0, len(g)), b.all(), pc.opts())


def _pile_norm(L, dirty):
    import test_pile_norm_gpu as tpn
    from gonomics_amd import align
    g, batch, opts, (plain, moved, plain_calls, moved_calls) = _pile_norm_case()
    L.set_reference(np.asarray(g, dtype=np.uint8))
    try:
        tpn._open_tracking(0, len(g))
        for part, _ in _halves(batch):
            dirty()
            tpn._add(tpn._params(), part)
        dirty()
        assert tpn._allele_tuples(L.pileup_alleles(normalize=True)) == moved
        t = L.get_timing()
        assert t["fast_path"] == 18 and t["cells"] == align.PileupAlleleInfo()["events"]
        dirty()
        assert tpn._calls(opts, True) == moved_calls and L.get_timing()["fast_path"] == 19
        dirty()
        assert tpn._calls(opts, False) == plain_calls
        assert tpn._allele_tuples(L.pileup_alleles()) == plain  # the log stays raw
    finally:
        _no_reference(L)


def _pile_qual(L, dirty):
    import test_pile_qual_gpu as tpq
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    batch, quals, (want, want_q) = tpq._seams(20)
    g = _pile_genome(L)
    try:
        align.PileupOpen(0, len(g))
        align.PileupTrackQualities(20)
        for part, q in _halves(batch, quals):
            dirty()
            tpq._add(tpg._params(), part, q)
            assert L.get_timing()["fast_path"] == 14
        dirty()
        got, got_q = tpq._both()
        assert not tpg._differences(got, want, 0), tpg._differences(got, want, 0)
        assert (got_q == want_q).all(), np.nonzero((got_q != want_q).any(axis=1))[0][:5]
    finally:
        _no_reference(L)


@functools.lru_cache(maxsize=None)
def _geno_case():
    import pyref_pile_qual as ref
    import test_pile_qual_gpu as tpq
    import test_summary_gpu as tsg
    g, _ = tsg._resident_cases()
    start, n = 48, 257
    batch, quals = tpq._site_batch(g, start, n, lambda k: tpq.CLASSES[(k * 5 + 1) % 7])
    pile = tpq._restate((start, n), batch, quals, 0)
    o = tpq.GENO_OPTS[0]
    want = tpq._want_tuples(ref.genotypes(pile, g[start:start + n], o, region_start=start))
    assert len(want) > 20
    return start, n, batch, quals, o, want


def _pile_genotypes(L, dirty):
    import test_pile_qual_gpu as tpq
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    start, n, batch, quals, o, want = _geno_case()
    _pile_genome(L)
    try:
        align.PileupOpen(start, n)
        align.PileupTrackQualities(0)
        for part, q in _halves(batch, quals):
            dirty()
            tpq._add(tpg._params(), part, q)
        dirty()
        got = L.pileup_genotypes(o["min_depth"], o["min_qual"], o["prior_het"], o["prior_hom"])
        assert tpq._geno_tuples(got) == want and (got["_pad"] == 0).all()
        t = L.get_timing()
        assert t["fast_path"] == 20 and t["cells"] == n
    finally:
        _no_reference(L)


for _form in ("0", "1"):
    ROUTES["pile/plain_adds/form%s" % _form] = Case({"GNX_PILE_FORM": _form}, _pile_plain, None)
    ROUTES["pile/tracking_adds_and_alleles/form%s" % _form] = Case({"GNX_PILE_FORM": _form}, _pile_alleles, None)
    ROUTES["pile/quality_adds/form%s" % _form] = Case({"GNX_PILE_FORM": _form}, _pile_qual, None)
ROUTES["pile/calls"] = Case({}, _pile_calls, None)
ROUTES["pile/alleles_norm_and_indel_calls"] = Case({}, _pile_norm, None)
ROUTES["pile/genotypes"] = Case({}, _pile_genotypes, None)


# ---- (a) the poisoned workspace ------------------------------------------------------------------------------------------------------------
RAN = set()
FILLED = {}


def _apply(monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("pattern", PATTERNS, ids=["%08x" % p for p in PATTERNS])
@pytest.mark.parametrize("key", list(ROUTES))
def test_poisoned_workspace(gpu_lib, monkeypatch, key, pattern):
    """run (the buffers have their size: a freshly grown one is cleared memory and proves nothing), fill, run again"""
    L = gpu_lib
    case = ROUTES[key]
    _apply(monkeypatch, case.env)

    def dirty():
        n_buffers, n_bytes = L.debug_fill_scratch(pattern)
        assert n_buffers > 0 and n_bytes > 0
        FILLED[key] = max(FILLED.get(key, 0), n_bytes)
    case.run(L, lambda: None)
    dirty()
    case.run(L, dirty)
    RAN.add((key, pattern))


def test_every_case_ran(request):
    """no case was skipped: the (route, pattern) cases that ran are those of the table (all of them, when the whole module was selected)"""
    assert len(PATTERNS) == 4 and len(ROUTES) >= 150
    selected = [it for it in request.session.items if getattr(it, "originalname", "") == "test_poisoned_workspace" and it.module.__name__ == __name__]
    assert len(RAN) == len(selected), (len(RAN), len(selected))
    if len(selected) == len(ROUTES) * len(PATTERNS):
        assert RAN == {(k, p) for k in ROUTES for p in PATTERNS}
    print("bytes filled per call, largest over the cases: %d; median %d" % (max(FILLED.values()), sorted(FILLED.values())[len(FILLED) // 2]))


def test_the_hook_fills_and_is_refused_without_the_switch(gpu_lib, monkeypatch):
    L = gpu_lib
    L.align_batch(L.make_params(0, ASYM, -600, -150), *asym.batch("small"))
    n_buffers, n_bytes = L.debug_fill_scratch(0x80808080)
    assert n_buffers >= 10 and n_bytes >= 4096
    monkeypatch.delenv("GNX_DEBUG_ENTRY")
    with pytest.raises(L.GnxError) as e:
        L.debug_fill_scratch(0)
    assert e.value.code == L.GNX_EINVAL


# ---- (b) the previous call's own data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALIGN_KEYS)
def test_previous_calls_data(gpu_lib, monkeypatch, key):
    """big, small, big' on one context with nothing in between: the small batch has the big one's live data behind its own extent, and
    big' finds the small one's in front of the first's"""
    case = ROUTES[key]
    _apply(monkeypatch, case.env)
    name, mode, go, ge, ci, route = case.align
    for which in ("big", "small", "other"):
        _align_once(gpu_lib, name, which, mode, go, ge, ci, route, key)


def test_chain_across_routes(gpu_lib, monkeypatch):
    """latency geometry, snapshot path, fast path, latency geometry: they share trace, hcol, rowbuf, dcol and plans"""
    steps = [({"GNX_LAT": "2"}, "tall12", 3), ({"GNX_CLONG": "2", "GNX_W64": "0"}, "long40", 2), ({"GNX_FASTPATH": "2"}, "fp2", 1), ({"GNX_LAT": "2"}, "small", 3),
             ({"GNX_CLONG": "2", "GNX_W64": "2"}, "w64", 6), ({"GNX_FASTPATH": "2"}, "fp3", 1), ({"GNX_LAT": "2"}, "tall12", 3)]
    for env, name, route in steps:
        with monkeypatch.context() as mp:
            _apply(mp, env)
            _align_once(gpu_lib, name, "big", 0, -600, -150, 10000, route, "chain")


def test_chain_drops_the_cached_plans(gpu_lib, monkeypatch):
    """every driver that writes `plans` takes the fast path's cached plans away: the SAME fast-path lengths before and after a call of
    the snapshot path (16 and 64 lanes), the row panels, the stored matrix and the latency geometry -- a miss each time, the oracle's
    result each time (a driver that overwrote `plans` and left the cache's pointer would hit, on the other driver's plans)"""
    L = gpu_lib
    between = [({"GNX_CLONG": "2", "GNX_W64": "0"}, "long40", 2), ({"GNX_MEGA_STRIPS": "2"}, "panels", 5), ({"GNX_FASTPATH": "0"}, "long16", 0),
               ({"GNX_CLONG": "2", "GNX_W64": "2"}, "w64", 6), ({"GNX_LAT": "2"}, "tall12", 3)]

    def fast(which):
        with monkeypatch.context() as mp:
            mp.setenv("GNX_FASTPATH", "2")
            L.debug_counter(12); L.debug_counter(13)
            _align_once(L, "fp2", which, 0, -600, -150, 10000, 1, "chain")
            return L.debug_counter(12), L.debug_counter(13)
    L.debug_fill_scratch(0)
    assert fast("big") == (0, 1) and fast("other") == (1, 0)  # (the cache works: equal lengths hit)
    for k, (env, name, route) in enumerate(between):
        with monkeypatch.context() as mp:
            _apply(mp, env)
            _align_once(L, name, "big", 0, -600, -150, 10000, route, "chain")
        assert fast("big" if k % 2 else "other") == (0, 1), (name, "left the cached plans standing")
        assert fast("other" if k % 2 else "big") == (1, 0)


# the forced certificate in (b): its flags, their scan, the live list and the live pairs' plans are what a smaller batch leaves data behind in
@functools.lru_cache(maxsize=None)
def _cert_variant(which):
    import test_fp_cert_gpu as tfc
    from gonomics_amd import _lib
    reads, wins, exp, _ = _cert_batch()
    if which == "small":  # half the pairs, every window a third shorter (300 -> 200, 2000 -> 1334 columns: still n + 2 and more)
        reads, wins = list(reads[:len(reads) // 2]), [np.ascontiguousarray(w[:len(w) - len(w) // 3]) for w in wins[:len(wins) // 2]]
    elif which == "other":  # the same lengths, other bases
        reads, wins = [np.ascontiguousarray(r[::-1]) for r in reads], [np.ascontiguousarray(w[::-1]) for w in wins]
    if which != "big":
        exp = oracle.align_batch(oracle.MODE_AFFINE, tfc.HCT, tfc.GO, tfc.GE, reads, wins, threads=8)
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, tfc.HCT, tfc.GO, tfc.GE)
    return reads, wins, exp, sum(1 for a, b in zip(reads, wins) if _lib.debug_gapless_certificate(p, a, b, K=16)[0])


def test_previous_calls_data_certificate(gpu_lib, monkeypatch):
    import test_fp_cert_gpu as tfc
    L = gpu_lib
    monkeypatch.setenv("GNX_FASTPATH", "2")
    monkeypatch.setenv("GNX_FP_CERT", "2")
    hosts = []
    for which in ("big", "small", "other"):
        reads, wins, exp, host = _cert_variant(which)
        hosts.append(host)
        L.debug_counter(9); L.debug_counter(10); L.debug_counter(11)
        got = L.align_batch(L.make_params(L.GNX_AFFINE_GAP, tfc.HCT, tfc.GO, tfc.GE), list(reads), list(wins))
        assert L.get_timing()["fast_path"] == 1
        common.assert_same(got, exp, "gapless certificate forced on, %s" % which)
        assert (L.debug_counter(9) + L.debug_counter(11), L.debug_counter(10)) == (host, len(reads)), which
    assert 0 < hosts[1] < len(_cert_variant("small")[0]) and 0 < hosts[0] < len(_cert_variant("big")[0])  # live lists neither empty nor everything


# ---- (c) the plan cache ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cache_batches(S):
    """X, X's lengths with other bases, X with one window one base longer, X's first half; each with the oracle's result"""
    reads, wins = variant("fp%d" % S, "big")
    reads2, wins2 = variant("fp%d" % S, "other")
    longer = list(wins)
    longer[5] = np.concatenate([wins[5], np.asarray([2], np.uint8)])
    h = len(reads) // 2
    out = {"X": (reads, wins), "X2": (reads2, wins2), "longer": (reads, longer), "half": (reads[:h], wins[:h])}
    res = {k: (a, b, oracle.align_batch(0, ASYM, -600, -150, a, b, threads=8)) for k, (a, b) in out.items()}
    res["X_local"] = (wins, reads, oracle.align_batch(3, ASYM, -600, -150, wins, reads, threads=8))
    res["X2_local"] = (wins2, reads2, oracle.align_batch(3, ASYM, -600, -150, wins2, reads2, threads=8))
    return res


@pytest.mark.parametrize("S", [1, 2, 3])
def test_plan_cache(gpu_lib, monkeypatch, S):
    """run_device_fp keeps the plans of the previous call on the device and skips their upload when the lengths (and the row blocks) are
    those of the previous call -- every step of a stream of equal-length batches after the first.  The cache holds ONE call: the call
    that returns to X's lengths after a miss is itself a miss, and the one after it hits."""
    L = gpu_lib
    B = _cache_batches(S)
    monkeypatch.setenv("GNX_FASTPATH", "2")

    def call(which, mode=0, route=1):
        a, b, exp = B[which]
        L.debug_counter(12); L.debug_counter(13)
        got = L.align_batch(L.make_params(mode, ASYM, -600, -150), list(a), list(b))
        _route_is(L.get_timing(), route, which)
        common.assert_same(got, exp, "plan cache, %d row blocks, %s" % (S, which))
        return L.debug_counter(12), L.debug_counter(13)  # (hits, misses) of this call
    L.debug_fill_scratch(0xFFFFFFFF)                     # whatever an earlier test cached is gone
    assert call("X") == (0, 1)                           # 1
    assert call("X2") == (1, 0)                          # 2: the cached branch, other bases
    assert call("longer") == (0, 1)                      # 3: the same pair count, one length differs
    assert call("X2") == (0, 1)                          # 4: X's lengths again -- the one entry holds step 3's
    assert call("X") == (1, 0)                           #    ... and now X's
    with monkeypatch.context() as mp:                    # 5: a latency-geometry call drops the cache
        mp.delenv("GNX_FASTPATH")
        mp.setenv("GNX_LAT", "2")
        _align_once(L, "small", "big", 0, -600, -150, 10000, 3, "between two fast-path calls")
    assert call("X") == (0, 1)                           # 6
    assert call("half") == (0, 1)                        # 7: fewer pairs
    assert call("X_local", mode=3) == (0, 1)             # 8: X's lengths through the transposed local entry
    assert call("X2_local", mode=3) == (1, 0)
    assert call("X") == (1, 0)                           # the key is rows, columns and row blocks: what the transposed call cached is X's
