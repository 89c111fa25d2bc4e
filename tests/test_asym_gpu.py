"""An asymmetric score matrix through every kernel route.  The C ABI takes any 5 x 5 table and the reference indexes it as
scores[alpha base][beta base] (align/affineGap.go:183, align/constGap.go:157, genomeGraph/search.go:246); every other GPU suite uses
symmetric, complement-invariant tables, on which a wrong (or forgotten) transpose of the table, a complement applied to the table
instead of the read, or the N row taken for the N column changes nothing.  Here every route -- forced with the switches the other suites
use and asserted through the timing's fast_path -- runs tests/asym.py's ASYM and must give the oracle's scores, offsets, runs and
ops bit for bit.  Every batch also satisfies asym.assert_tells_orientation: the oracle itself scores at least half of its pairs
differently under the transposed (or complemented) table, so no case passes vacuously (tests/test_asym_cpu.py checks the same
without a GPU, and that the oracle's own orientation is the pure-Python statements')."""
import numpy as np
import pytest

import asym
import common
import oracle
import pyref_span
from asym import ASYM, ASYM_RC, ASYM_T

pytestmark = pytest.mark.gpu

LOWMEM = (0, 1)
ROUTE_SWITCHES = ("GNX_FASTPATH", "GNX_NO_HFORM", "GNX_LAT", "GNX_WIDE", "GNX_CLONG", "GNX_W64", "GNX_REBASE", "GNX_CL_CKC", "GNX_MEGA_STRIPS",
                  "GNX_W64_FARM", "GNX_W64_SPEC", "GNX_W64_FARM_PIPE", "GNX_W64_CK", "GNX_FP_MAXIT", "GNX_TB_TWO_PASS", "GNX_SCORE_SWEEP", "GNX_NO_PIPE")


@pytest.fixture(autouse=True)
def _own_switches(monkeypatch):
    """the routes are this module's to choose: every case starts without the switches (tools/switch_matrix.sh sets some from outside)"""
    for k in ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _align(L, name, mode, go, ge, route, mname="ASYM", ci=10000, what=""):
    """a named batch through align_batch under the switches in force: the oracle's bits, the route asked for, and a batch that tells"""
    alphas, betas = asym.batch(name)
    if mname == "ASYM" and (go, ge) in asym.pens(mode):
        assert asym.tells(name, mode, go, ge, ci=ci)
    got = L.align_batch(L.make_params(mode, asym.MATRICES[mname], go, ge, ci, ci), alphas, betas)
    tm = L.get_timing()
    common.assert_same(got, asym.expected(name, mode, mname, go, ge, ci), "%s %s mode %d (%d, %d) checkersize %d %s" % (name, mname, mode, go, ge, ci, what))
    if route in (0, 1, 2):
        common.expect_route(tm, route)
    elif route is not None and not common.OUTER_ROUTE_SWITCH:
        assert tm["fast_path"] == route, (tm["fast_path"], route, name, mode, what)
    return tm


# ---- route 0: the stored direction matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["rebased", "plain"])
@pytest.mark.parametrize("mode", range(5))
def test_stored_matrix(gpu_lib, monkeypatch, mode, table):
    """fill_affine_kernel / fill_const_kernel + traceback_kernel: one strip (64 pairs) and several 160-row strips (16 pairs up to 700 x 1500),
    with the rebased tables (h-form) and with the plain ones (GNX_NO_HFORM)"""
    monkeypatch.setenv("GNX_FASTPATH", "0")
    if table == "plain":
        monkeypatch.setenv("GNX_NO_HFORM", "1")
    for go, ge in asym.pens(mode):
        for name in ("small", "long16"):
            _align(gpu_lib, name, mode, go, ge, 0, what=table)
            if mode in LOWMEM:
                _align(gpu_lib, name, mode, go, ge, 0, ci=7, what=table)
        _align(gpu_lib, "small", mode, go, ge, 0, mname="ASYM_T", what=table)


@pytest.mark.parametrize("mode", range(5))
def test_stored_matrix_cooperative_traceback(gpu_lib, monkeypatch, mode):
    """beta >= 1024: the strips of a pair as pipelined workgroups, the walk by one wave per pair -- in one pass and as count + write"""
    monkeypatch.setenv("GNX_FASTPATH", "0")
    go, ge = asym.pens(mode)[-1]
    _align(gpu_lib, "coop", mode, go, ge, 0)
    monkeypatch.setenv("GNX_TB_TWO_PASS", "1")
    _align(gpu_lib, "coop", mode, go, ge, 0, what="two-pass walk")


# ---- route 1: the affine fast path, and its transposed form for AffineGapLocal ----------------------------------------------------------
@pytest.mark.parametrize("local", [False, True], ids=["global", "transposed"])
@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_fast_path(gpu_lib, monkeypatch, blocks, local):
    """fp_sweep_kernel + fp_walk_kernel with reads of one, two and three 160-row blocks against windows of 128 .. 2049 columns;
    AffineGapLocal(target = window, query = read) runs the same sweep on the transposed problem with a table the host transposes"""
    monkeypatch.setenv("GNX_FASTPATH", "2")
    mode, name = (3, "xp%d" % blocks) if local else (0, "fp%d" % blocks)
    for go, ge in asym.AFFINE_PENS:
        _align(gpu_lib, name, mode, go, ge, 1)
    if blocks < 3:
        _align(gpu_lib, name, mode, -600, -150, 1, mname="ASYM_T")
    if blocks == 2 and not local:  # checkerboard edges inside the windows; windows re-filled by fill_affine, stragglers through fp_walk
        for maxit in (None, "0", "3"):
            if maxit is not None:
                monkeypatch.setenv("GNX_FP_MAXIT", maxit)
            _align(gpu_lib, name, mode, -600, -150, None, ci=7, what="maxit %s" % maxit)


@pytest.mark.parametrize("local", [False, True], ids=["global", "transposed"])
def test_fast_path_overflow_redo(gpu_lib, monkeypatch, local):
    """gaps as cheap as (-30, -10): a few CIGARs exceed the 64 runs the fast path stages and are aligned again on the general path --
    for the transposed form in the original orientation, with the table as the caller gave it"""
    monkeypatch.setenv("GNX_FASTPATH", "2")
    mode, name = (3, "xp_cheap") if local else (0, "fp_cheap")
    go, ge = asym.CHEAP_GAPS
    assert asym.tells(name, mode, go, ge)
    runs = np.diff(asym.expected(name, mode, "ASYM", go, ge)[2])
    assert 1 <= int(np.sum(runs > 64)) <= len(runs) // 2
    _align(gpu_lib, name, mode, go, ge, 1)


# ---- routes 3 and 4: the latency geometry and the int64 kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(5))
def test_latency_geometry(gpu_lib, monkeypatch, mode):
    """GNX_LAT=2: lat_fill_kernel (one pair per wave, 64 lanes x 2 rows) whatever the batch: one strip, and tall pairs of many strips"""
    monkeypatch.setenv("GNX_LAT", "2")
    for go, ge in asym.pens(mode):
        for name in ("small", "tall12"):
            _align(gpu_lib, name, mode, go, ge, 3)
    _align(gpu_lib, "small", mode, *asym.pens(mode)[0], 3, mname="ASYM_T")


@pytest.mark.parametrize("mode", range(5))
def test_int64_kernel(gpu_lib, monkeypatch, mode):
    """GNX_WIDE=2: lat_wide_kernel (literal recurrences on int64 keys), also with gapOpen = +25, which no other kernel takes, and 0.
    (Where a one-base gap costs 5, nothing, or pays, no mismatch survives in an optimal alignment: those runs cannot tell a table
    from its transpose -- the named penalty sets on the same batch do.)"""
    monkeypatch.setenv("GNX_WIDE", "2")
    affine = mode in asym.AFFINE_MODES
    for go, ge in asym.pens(mode) + ([(25, -30), (0, -150)] if affine else [(25, 0), (0, 0)]):
        _align(gpu_lib, "small", mode, go, ge, 4)
    _align(gpu_lib, "long16", mode, *asym.pens(mode)[-1], 4)
    _align(gpu_lib, "small", mode, *asym.pens(mode)[0], 4, mname="ASYM_T")


# ---- routes 2 and 6: score-only sweep with snapshots, fused re-fill + walk ---------------------------------------------------------------
@pytest.mark.parametrize("rebase", [False, True], ids=["static", "rebase"])
@pytest.mark.parametrize("mode,cs", [(0, 3), (0, 10000), (1, 3), (1, 10000), (2, 10000), (4, 10000)])
def test_snapshot_path_16_lanes(gpu_lib, monkeypatch, mode, cs, rebase):
    """GNX_CLONG=2, GNX_W64=0: affine_long / const_long (al_sweep, cl_sweep_wg, cl_walk), absolute keys and moving bases"""
    monkeypatch.setenv("GNX_CLONG", "2")
    monkeypatch.setenv("GNX_W64", "0")
    if rebase:
        monkeypatch.setenv("GNX_REBASE", "1")
    for go, ge in asym.pens(mode):
        _align(gpu_lib, "long40", mode, go, ge, 2, ci=cs)
    if mode in (1, 4):
        monkeypatch.setenv("GNX_CL_CKC", "224")
        _align(gpu_lib, "long40", mode, asym.CONST_GAP, 0, 2, ci=cs, what="snapshot spacing 224")
        monkeypatch.delenv("GNX_CL_CKC")
    if cs == 10000 and not rebase:
        _align(gpu_lib, "long40", mode, *asym.pens(mode)[0], 2, mname="ASYM_T")


@pytest.mark.parametrize("walk", ["farm", "two_waves", "one_wave"])
@pytest.mark.parametrize("mode,cs", [(0, 16), (0, 10000), (1, 16), (1, 10000), (2, 10000), (4, 10000)])
def test_snapshot_path_64_lanes(gpu_lib, monkeypatch, mode, cs, walk):
    """GNX_CLONG=2, GNX_W64=2: affine_long64 / const_long64 with the walk as a farm (farm64.hip.h), on one workgroup of two waves, or on
    one wave; pairs of up to 2000 x 1500, a third of them of two or more 640-row strips"""
    monkeypatch.setenv("GNX_CLONG", "2")
    monkeypatch.setenv("GNX_W64", "2")
    if walk != "farm":
        monkeypatch.setenv("GNX_W64_FARM", "0")
    if walk == "one_wave":
        monkeypatch.setenv("GNX_W64_SPEC", "0")
    assert sum(1 for a in asym.batch("w64")[0] if len(a) > 1280) >= 4 and len(asym.batch("w64")[0]) == 12
    for go, ge in asym.pens(mode):
        _align(gpu_lib, "w64", mode, go, ge, 6, ci=cs, what=walk)
    if cs == 10000 and walk == "farm":
        _align(gpu_lib, "w64", mode, *asym.pens(mode)[0], 6, mname="ASYM_T", what=walk)


# ---- route 5: row panels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["16", "64"])
@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_row_panels(gpu_lib, monkeypatch, mode, lanes):
    """GNX_MEGA_STRIPS=2: run_device_mega, forward and backward panels of two strips (of 160 rows, and of 640 with GNX_W64=2)"""
    monkeypatch.setenv("GNX_MEGA_STRIPS", "2")
    if lanes == "64":
        monkeypatch.setenv("GNX_W64", "2")
    for go, ge in asym.pens(mode):
        for cs in ((1000, 10000) if mode in LOWMEM else (10000,)):
            _align(gpu_lib, "panels", mode, go, ge, 5, ci=cs, what=lanes + " lanes")
    if lanes == "16":
        _align(gpu_lib, "panels", mode, *asym.pens(mode)[-1], 5, mname="ASYM_T")


# ---- route 7: the score sweep --------------------------------------------------------------------------------------------------------
def _scores(mode, mname, go, ge, name="sweep"):
    return np.asarray(asym.expected(name, mode, mname, go, ge)[0], dtype=np.int64)


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_score_sweep(gpu_lib, monkeypatch, mode):
    """score_batch on a batch that holds pairs with n < m and pairs with n > m (ScorePlan::swap takes both values inside one launch),
    the shorter side 1 .. 400 (one to three levels); then the align route with the CIGAR dropped"""
    alphas, betas = asym.batch("sweep")
    assert any(len(a) < len(b) for a, b in zip(alphas, betas)) and any(len(a) > len(b) for a, b in zip(alphas, betas))
    for k, (go, ge) in enumerate(asym.pens(mode)):
        assert asym.tells("sweep", mode, go, ge)
        for mname in (("ASYM", "ASYM_T") if k == 0 else ("ASYM",)):
            p = gpu_lib.make_params(mode, asym.MATRICES[mname], go, ge)
            got = gpu_lib.score_batch(p, alphas, betas)
            assert gpu_lib.get_timing()["fast_path"] == 7
            exp = _scores(mode, mname, go, ge)
            assert np.array_equal(got, exp), (mname, go, np.flatnonzero(got != exp)[:8])
            assert np.array_equal(got, gpu_lib.align_batch(p, alphas, betas)[0])
    monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
    go, ge = asym.pens(mode)[0]
    got = gpu_lib.score_batch(gpu_lib.make_params(mode, ASYM, go, ge), alphas, betas)
    assert gpu_lib.get_timing()["fast_path"] != 7
    assert np.array_equal(got, _scores(mode, "ASYM", go, ge))


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_score_sweep_by_offset(gpu_lib, mode):
    """the same shapes against windows of a packed resident reference with N (the windows are the kernels' beta)"""
    ref, reads, w_start, w_len = asym.global_ref_batch()
    wins = [ref[s:s + l] for s, l in zip(w_start, w_len)]
    cat = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    gpu_lib.set_reference(ref)
    try:
        for go, ge in asym.pens(mode):
            exp = asym.assert_tells_orientation(mode, go, ge, reads, wins)
            p = gpu_lib.make_params(mode, ASYM, go, ge)
            got = gpu_lib.score_batch_by_offset(p, cat, off, w_start, w_len)
            assert gpu_lib.get_timing()["fast_path"] == 7
            assert np.array_equal(got, exp[0]), np.flatnonzero(got != exp[0])[:8]
            common.assert_same(gpu_lib.align_batch_by_offset(p, cat, off, w_start, w_len), exp, "align twin by offset, mode %d" % mode)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- routes 8 and 10: the local score sweep, target end and target span ------------------------------------------------------------------
@pytest.fixture(scope="module")
def local_spans():
    targets, queries = asym.batch("local")
    return {(mname, go, ge): pyref_span.spans_from_oracle(asym.MATRICES[mname], go, ge, targets, queries, threads=8)
            for mname, go, ge in [("ASYM", -400, -30), ("ASYM", -600, -150), ("ASYM_T", -400, -30), ("ASYM", 25, -30), ("ASYM", -400, 0)]}


def _local_tables():
    ref, t_start, t_len, queries = asym.local_ref_batch()
    q_cat = np.concatenate(queries)
    q_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    return ref, t_start, t_len, q_cat, q_off


@pytest.mark.parametrize("mname,go,ge", [("ASYM", -400, -30), ("ASYM", -600, -150), ("ASYM_T", -400, -30)])
def test_locate_and_span(gpu_lib, local_spans, mname, go, ge):
    """locate_batch / _windows / _by_offset (route 8) and locate_span_batch / _by_offset (route 10) against the oracle's AffineGapLocal:
    its score, its leading ColD run, the target length minus its trailing ColD run.  _by_offset has the queries as the kernels' alpha
    and transposes the table on the host; queries of up to 192 bases and of 193 .. 400 (row hand-over in device memory); targets
    shorter than their query.  Any GnxError -- GNX_ETRACE, the span kernel's self-check, among them -- fails the test."""
    targets, queries = asym.batch("local")
    ref, t_start, t_len, q_cat, q_off = _local_tables()
    if mname == "ASYM":
        assert asym.tells("local", 3, go, ge)
    S, start, end = local_spans[(mname, go, ge)]
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, asym.MATRICES[mname], go, ge)
    gpu_lib.set_reference(ref)
    try:
        calls = [("locate_batch", 8, lambda: gpu_lib.locate_batch(p, targets, queries)),
                 ("locate_batch_windows", 8, lambda: gpu_lib.locate_batch_windows(p, ref, t_start, t_len, q_cat, q_off[:-1], np.diff(q_off))),
                 ("locate_batch_by_offset", 8, lambda: gpu_lib.locate_batch_by_offset(p, q_cat, q_off, t_start, t_len)),
                 ("locate_span_batch", 10, lambda: gpu_lib.locate_span_batch(p, targets, queries)),
                 ("locate_span_batch_by_offset", 10, lambda: gpu_lib.locate_span_batch_by_offset(p, q_cat, q_off, t_start, t_len))]
        for what, route, fn in calls:
            out = fn()
            assert gpu_lib.get_timing()["fast_path"] == route, (what, gpu_lib.get_timing()["fast_path"])
            assert np.array_equal(out[0], S), (what, "score", np.flatnonzero(out[0] != S)[:8])
            assert np.array_equal(out[-1], end), (what, "end", np.flatnonzero(out[-1] != end)[:8])
            if route == 10:
                assert np.array_equal(out[1], start), (what, "start", np.flatnonzero(out[1] != start)[:8])
        got = gpu_lib.score_batch(p, targets, queries)
        assert gpu_lib.get_timing()["fast_path"] == 8 and np.array_equal(got, S)
        assert np.array_equal(S, gpu_lib.align_batch(p, targets, queries)[0])
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    assert np.any(start > 0) and np.any(end < t_len)


@pytest.mark.parametrize("how", ["gapOpen > 0", "gapExtend = 0", "GNX_SCORE_SWEEP=0"])
def test_locate_and_span_fallbacks(gpu_lib, monkeypatch, local_spans, how):
    """what the local sweep does not take runs the align route -- for _by_offset with the two sides swapped back on the host --
    and the end (and start) are read off its CIGAR"""
    targets, queries = asym.batch("local")
    ref, t_start, t_len, q_cat, q_off = _local_tables()
    go, ge = {"gapOpen > 0": (25, -30), "gapExtend = 0": (-400, 0), "GNX_SCORE_SWEEP=0": (-400, -30)}[how]
    if how == "GNX_SCORE_SWEEP=0":
        monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
    S, start, end = local_spans[("ASYM", go, ge)]
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, ASYM, go, ge)
    gpu_lib.set_reference(ref)
    try:
        for what, fn in [("locate_batch", lambda: gpu_lib.locate_batch(p, targets, queries)),
                         ("locate_batch_by_offset", lambda: gpu_lib.locate_batch_by_offset(p, q_cat, q_off, t_start, t_len)),
                         ("locate_span_batch", lambda: gpu_lib.locate_span_batch(p, targets, queries)),
                         ("locate_span_batch_by_offset", lambda: gpu_lib.locate_span_batch_by_offset(p, q_cat, q_off, t_start, t_len))]:
            out = fn()
            if how != "gapExtend = 0":  # (gapExtend = 0 is the sweep's still; its span has no window bound)
                assert gpu_lib.get_timing()["fast_path"] not in (8, 10), (what, how)
            assert np.array_equal(out[0], S) and np.array_equal(out[-1], end), (what, how)
            if len(out) == 3:
                assert np.array_equal(out[1], start), (what, how, np.flatnonzero(out[1] != start)[:8])
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- N1: chunk and multiple alignment, align and score twins -----------------------------------------------------------------------------
def _n1_got(sc, ops, off, k):
    return (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])


@pytest.mark.parametrize("how", ["lat", "general", "sweep_off", "int64"])
@pytest.mark.parametrize("chunk", [1, 3, 5])
def test_affine_gap_chunk(gpu_lib, monkeypatch, chunk, how):
    """affine_gap_chunk_batch (explicit score matrices through lat_fill / fill_affine / lat_wide <SCORED>) and its score twin (route 9:
    the register-walking pairs kernel for chunks of 1 and 3, the generic one for 5), on pairs with nc > mc and pairs with nc < mc in
    one batch: the score sweep swaps the sides of the latter and reads a transposed table"""
    if how == "lat":
        monkeypatch.delenv("GNX_FP_SMALL", raising=False)  # the shipped routing: small batches in the latency geometry
    elif how == "general":
        monkeypatch.setenv("GNX_LAT", "0")
    elif how == "sweep_off":
        monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
    else:
        monkeypatch.setenv("GNX_WIDE", "2")
    alphas, betas = asym.chunk_pairs(chunk)
    assert any(len(a) > len(b) for a, b in zip(alphas, betas)) and any(len(a) < len(b) for a, b in zip(alphas, betas))
    for go, ge, mx in [(-400, -30, ASYM), (-600, -150, ASYM), (-400, -30, ASYM_T)]:
        if mx is ASYM:
            exp = asym.assert_tells_orientation(("chunk", chunk), go, ge, alphas, betas)
        else:
            exp = [oracle.affine_gap_chunk(mx, go, ge, chunk, a, b) for a, b in zip(alphas, betas)]
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, mx, go, ge)
        sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
        twin_route = gpu_lib.get_timing()["fast_path"]
        for k in range(len(alphas)):
            assert _n1_got(sc, ops, off, k) == exp[k], (chunk, how, go, k)
        got = gpu_lib.affine_gap_chunk_score_batch(p, chunk, alphas, betas)
        route = gpu_lib.get_timing()["fast_path"]
        assert [int(x) for x in got] == [e[0] for e in exp], (chunk, how, go)
        if not common.OUTER_ROUTE_SWITCH:
            assert (route == 9) if how in ("lat", "general") else (route == twin_route != 9), (how, route, twin_route)


@pytest.mark.parametrize("chunk", [1, 2])
def test_multiple_affine_gap(gpu_lib, monkeypatch, chunk):
    """groups of 1 .. 4 members with lower case and gaps, every pair as (x, y) and as (y, x): the column profiles
    wB[v][a] = sum_b scores[a][b] * cntB[v][b] are built for one orientation of the table"""
    blocks, pairs = asym.groups(chunk)
    assert all((y, x) in pairs for x, y in pairs)
    for go, ge, mx in [(-400, -30, ASYM), (-600, -150, ASYM), (-400, -30, ASYM_T)]:
        A, B = [blocks[x] for x, _ in pairs], [blocks[y] for _, y in pairs]
        if mx is ASYM:
            exp = asym.assert_tells_orientation(("multi", chunk), go, ge, A, B)
        else:
            exp = [oracle.multiple_affine_gap(mx, go, ge, chunk, a, b) for a, b in zip(A, B)]
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, mx, go, ge)
        for geometry in ("general", "lat"):
            if geometry == "lat":
                monkeypatch.delenv("GNX_FP_SMALL", raising=False)
            else:
                monkeypatch.setenv("GNX_FP_SMALL", "1")
            sc, ops, off = gpu_lib.multiple_affine_gap_batch(p, chunk, blocks, pairs)
            for k in range(len(pairs)):
                assert _n1_got(sc, ops, off, k) == exp[k], (chunk, geometry, go, pairs[k])
        got = gpu_lib.multiple_affine_gap_score_batch(p, chunk, blocks, pairs)
        assert common.OUTER_ROUTE_SWITCH or gpu_lib.get_timing()["fast_path"] == 9
        assert [int(x) for x in got] == [e[0] for e in exp], (chunk, go)


# ---- best of K on both strands -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(5))
def test_best_of(gpu_lib, mode):
    """best_of_windows and best_of_by_offset: the device reverse-complements the READ; the table stays as it is.  Expected values: the
    oracle on the flattened pair list with the reverse complement taken on the host (tests/test_best_of_gpu.py's _expected)"""
    import test_best_of_gpu as bo
    reads, target, cands = asym.best_of_workload()
    alphas, betas = bo._flatten(mode, reads, target, cands)
    for k, (go, ge) in enumerate(asym.pens(mode)):
        asym.assert_tells_orientation(mode, go, ge, alphas, betas, other=ASYM_RC)
        ck = 37 if (mode in LOWMEM and k == 0) else 10000
        p = gpu_lib.make_params(mode, ASYM, go, ge, ck, ck)
        exp = bo._expected(mode, ASYM, go, ge, reads, target, cands, ck, ck)
        assert sum(1 for cs, b in zip(cands, exp["best"]) if cs[b][2] == 1) >= 5 and any(b > 0 for b in exp["best"])  # winners on strand 1
        bo._check(bo._call(gpu_lib, p, reads, target, cands, cigar=True), exp, mode, True, "best_of_windows")
        if mode in (0, 1, 2, 4):
            assert gpu_lib.get_timing()["n_contexts"] == 1
        gpu_lib.set_reference(target)
        try:
            bo._check(bo._call(gpu_lib, p, reads, None, cands, cigar=True, resident=True), exp, mode, True, "best_of_by_offset")
            bo._check(bo._call(gpu_lib, p, reads, None, cands, cigar=False, resident=True), exp, mode, False, "best_of_by_offset, no CIGAR stage")
            assert gpu_lib.get_timing()["fast_path"] == (8 if mode == 3 else 7)
        finally:
            gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- the graph aligner -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [0, 1])
def test_gsw_extend(gpu_lib, side):
    """gsw_extend_batch, LeftDynamicAln and RightDynamicAln: score, end cell and route of the oracle's restatement"""
    from gonomics_amd import cigar, genomeGraph
    pairs = asym.gsw_pairs(side)
    alphas, betas = [a for a, _ in pairs], [b for _, b in pairs]
    exp = asym.assert_tells_orientation(("gsw", side), asym.GSW_GAP, 0, alphas, betas)
    got = genomeGraph.DynamicAlnBatch("left" if side == 0 else "right", alphas, betas, ASYM, asym.GSW_GAP)
    for k, ((score, route, i, j), (es, er, ei, ej)) in enumerate(zip(got, exp)):
        assert (score, i, j) == (es, ei, ej), (side, k, len(alphas[k]), len(betas[k]))
        assert [(c.RunLength, c.Op) for c in route] == [(r, cigar.from_col(o)) for r, o in er], (side, k)


@pytest.mark.parametrize("kind", ["linear", "wide"])
def test_gsw_map_reads(gpu_lib, kind):
    """gnx_gsw_map_reads on one small graph, reads of both strands: every Giraf equals the sequential restatement on the CPU oracle
    (tests/pyref_gsw.py).  The seeds' own score is a sum over the table's diagonal of the read as mapped, so a table complemented
    with the read shows in nearly every mapped read."""
    import pyref_gsw as ref
    import test_gsw_reads as tg
    from gonomics_amd import genomeGraph as gg
    seqs, edges, reads = tg.make_case(17, kind)
    g = tg.build(seqs, edges)
    nodes = ref.make_graph(seqs, edges)
    full = ref.index_genome(nodes, 16, 1)
    bigs = [gg.FastqBig("r%d" % k, rd) for k, rd in enumerate(reads)]
    ng = gg.NativeGraph(g, 16, 1)
    try:
        got = ng.GswBatchToGiraf(bigs, ASYM, on_panic="mark")
    finally:
        ng.handle.close()
    mapped = differ = minus = 0
    for k, rd in enumerate(reads):
        r2 = ref.make_read(rd)
        seeds = ref.seed_map(full, nodes, r2, 16)
        exp = ref.read_to_giraf(nodes, r2, seeds, ASYM)
        assert not isinstance(got[k], gg.GoPanic) and got[k].key() == ref.giraf_key(exp), "read %d" % k
        if exp["AlnScore"] > 0:
            mapped += 1
            minus += not exp["PosStrand"]
            differ += ref.read_to_giraf(nodes, r2, seeds, ASYM_RC)["AlnScore"] != exp["AlnScore"]
    assert mapped >= len(reads) // 2 and minus >= 5 and mapped - minus >= 5
    assert 2 * differ >= mapped, (differ, mapped)
