"""Tie-breaking at every argmax site, through every CIGAR route.  The reference's tripleMaxTrace prefers M over I over D -- in the three
recurrences, in the final state, in the restart after an upward exit of a checkerboard (quirk Q1) and in the constant-gap argmax --
and the kernels implement that many times over: as tag bits under the keys (fill_affine / fill_const + traceback, lat_fill, the
snapshot kernels), as literal compares (lat_wide), as arguments (fp_walk's shortcuts).  The other suites' penalty sets never let I and
D tie above M, so a kernel that prefers D passes them.  Here every route -- forced with the switches the other suites use, asserted
through the timing's fast_path -- runs tests/ties.py's sets (two gaps beat, or equal, a mismatch) on its batches and must give the
oracle's scores, offsets, runs and ops bit for bit.  Before each run ties.decisive holds: by the census of the reference's own route
an I/D tie lies on at least half of the pairs and every required class (site, tied set) on at least three -- at such a cell another
order of preference gives another CIGAR (tests/test_ties_cpu.py shows both without a GPU)."""
import numpy as np
import pytest

import common
import ties

pytestmark = pytest.mark.gpu

LOWMEM = (0, 1)
ROUTE_SWITCHES = ("GNX_FASTPATH", "GNX_NO_HFORM", "GNX_LAT", "GNX_WIDE", "GNX_CLONG", "GNX_W64", "GNX_REBASE", "GNX_CL_CKC", "GNX_MEGA_STRIPS",
                  "GNX_W64_FARM", "GNX_W64_SPEC", "GNX_W64_FARM_PIPE", "GNX_W64_CK", "GNX_FP_MAXIT", "GNX_TB_TWO_PASS", "GNX_SCORE_SWEEP", "GNX_NO_PIPE")


@pytest.fixture(autouse=True)
def _own_switches(monkeypatch):
    """the routes are this module's to choose: every case starts without the switches (tools/switch_matrix.sh sets some from outside)"""
    for k in ROUTE_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _align(L, name, mode, sname, route, ci=10000, what=""):
    """a named batch through align_batch under the switches in force: a batch on which the ties decide, the oracle's bits, the route asked for"""
    alphas, betas = ties.batch(name)
    assert ties.diag_condition(sname) if name == "diag" else ties.decisive(name, mode, sname, ci)
    table, go, ge = ties.params(mode, sname)
    got = L.align_batch(L.make_params(mode, table, go, ge, ci, ci), alphas, betas)
    tm = L.get_timing()
    common.assert_same(got, ties.expected(name, mode, sname, ci), "%s mode %d %s (%d, %d) checkersize %d %s" % (name, mode, sname, go, ge, ci, what))
    if route in (0, 1, 2):
        common.expect_route(tm, route)
    elif route is not None and not common.OUTER_ROUTE_SWITCH:
        assert tm["fast_path"] == route, (tm["fast_path"], route, name, mode, what)
    return tm


# ---- route 0: the stored direction matrix ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["rebased", "plain"])
@pytest.mark.parametrize("mode", range(5))
def test_stored_matrix(gpu_lib, monkeypatch, mode, table):
    """fill_affine_kernel / fill_const_kernel + traceback_kernel: one strip and several 160-row strips, the rebased tables (h-form) and
    the plain ones (GNX_NO_HFORM); 7 x 7 checkerboards in the low-memory modes (Q1 on every seventh row)"""
    monkeypatch.setenv("GNX_FASTPATH", "0")
    if table == "plain":
        monkeypatch.setenv("GNX_NO_HFORM", "1")
    for name in ("small", "long16"):
        for sname in ties.plan_sets(name, mode):
            for ci in ties.checkers(name, mode):
                _align(gpu_lib, name, mode, sname, 0, ci=ci, what=table)


@pytest.mark.parametrize("mode", range(5))
def test_stored_matrix_cooperative_traceback(gpu_lib, monkeypatch, mode):
    """beta >= 1024: the strips of a pair as pipelined workgroups, the walk by one wave per pair -- in one pass and as count + write"""
    monkeypatch.setenv("GNX_FASTPATH", "0")
    for sname in ties.plan_sets("coop", mode):
        _align(gpu_lib, "coop", mode, sname, 0)
    monkeypatch.setenv("GNX_TB_TWO_PASS", "1")
    for sname in ties.plan_sets("coop", mode):
        _align(gpu_lib, "coop", mode, sname, 0, what="two-pass walk")


# ---- routes 3 and 4: the latency geometry and the int64 kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(5))
def test_latency_geometry(gpu_lib, monkeypatch, mode):
    """GNX_LAT=2: lat_fill_kernel (one pair per wave, 64 lanes x 2 rows): one strip, and tall pairs of many 128-row strips"""
    monkeypatch.setenv("GNX_LAT", "2")
    for name in ("small", "tall12"):
        for sname in ties.plan_sets(name, mode):
            _align(gpu_lib, name, mode, sname, 3)


@pytest.mark.parametrize("mode", range(5))
def test_int64_kernel(gpu_lib, monkeypatch, mode):
    """GNX_WIDE=2: lat_wide_kernel, whose recurrences are literal three-way compares on int64 values"""
    monkeypatch.setenv("GNX_WIDE", "2")
    for name in ("small", "long16"):
        for sname in ties.plan_sets(name, mode):
            _align(gpu_lib, name, mode, sname, 4)


# ---- routes 2 and 6: score-only sweep with snapshots, fused re-fill + walk ---------------------------------------------------------------
@pytest.mark.parametrize("rebase", [False, True], ids=["static", "rebase"])
@pytest.mark.parametrize("mode,cs", [(0, 3), (0, 10000), (1, 3), (1, 10000), (2, 10000), (4, 10000)])
def test_snapshot_path_16_lanes(gpu_lib, monkeypatch, mode, cs, rebase):
    """GNX_CLONG=2, GNX_W64=0: affine_long / const_long (al_sweep, cl_sweep_wg, cl_walk) on absolute keys and on moving bases; both
    snapshot spacings of the constant-gap sweep; the walk without and with three speculative tiles"""
    monkeypatch.setenv("GNX_CLONG", "2")
    monkeypatch.setenv("GNX_W64", "0")
    if rebase:
        monkeypatch.setenv("GNX_REBASE", "1")
    sets_ = ties.plan_sets("long40", mode)
    for sname in sets_:
        _align(gpu_lib, "long40", mode, sname, 2, ci=cs)
    if mode in (1, 4):
        for ckc in ("224", "448"):
            monkeypatch.setenv("GNX_CL_CKC", ckc)
            _align(gpu_lib, "long40", mode, sets_[0], 2, ci=cs, what="snapshot spacing " + ckc)
        monkeypatch.delenv("GNX_CL_CKC")
    for spec in ("0", "3"):
        monkeypatch.setenv("GNX_CL_WALK_SPEC", spec)
        for sname in sets_:
            _align(gpu_lib, "long40", mode, sname, 2, ci=cs, what="walk spec " + spec)


@pytest.mark.parametrize("walk", ["farm", "farm1", "two_waves", "one_wave"])
@pytest.mark.parametrize("mode,cs", [(0, 16), (0, 10000), (1, 16), (1, 10000), (2, 10000), (4, 10000)])
def test_snapshot_path_64_lanes(gpu_lib, monkeypatch, mode, cs, walk):
    """GNX_CLONG=2, GNX_W64=2: affine_long64 / const_long64 with the walk as a farm (farm64.hip.h; at its own width and with one tile),
    on one workgroup of two waves, or on one wave; four of the ten pairs of two or more 640-row strips"""
    monkeypatch.setenv("GNX_CLONG", "2")
    monkeypatch.setenv("GNX_W64", "2")
    if walk == "farm1":
        monkeypatch.setenv("GNX_W64_FARM", "1")
    elif walk != "farm":
        monkeypatch.setenv("GNX_W64_FARM", "0")
    if walk == "one_wave":
        monkeypatch.setenv("GNX_W64_SPEC", "0")
    for sname in ties.plan_sets("w64", mode):
        _align(gpu_lib, "w64", mode, sname, 6, ci=cs, what=walk)


# ---- route 5: row panels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["16", "64"])
@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_row_panels(gpu_lib, monkeypatch, mode, lanes):
    """GNX_MEGA_STRIPS=2: run_device_mega, forward and backward panels of two strips (of 160 rows, and of 640 with GNX_W64=2)"""
    monkeypatch.setenv("GNX_MEGA_STRIPS", "2")
    if lanes == "64":
        monkeypatch.setenv("GNX_W64", "2")
    for sname in ties.plan_sets("panels", mode):
        for cs in ties.checkers("panels", mode):
            _align(gpu_lib, "panels", mode, sname, 5, ci=cs, what=lanes + " lanes")


# ---- route 1: the affine fast path, and its transposed form for AffineGapLocal ----------------------------------------------------------
@pytest.mark.parametrize("local", [False, True], ids=["global", "transposed"])
@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_fast_path(gpu_lib, monkeypatch, blocks, local):
    """fp_sweep_kernel + fp_walk_kernel with reads of one, two and three 160-row blocks in windows of about their length; by the
    oracle's run counts at most half of the CIGARs exceed the 64 runs the walk stages (ties.staged) -- those few are aligned again on
    the general path, and must come out the same.  Then the walk with one lane per pair"""
    monkeypatch.setenv("GNX_FASTPATH", "2")
    mode, name = (3, "xp%d" % blocks) if local else (0, "fp%d" % blocks)
    for sname in ties.plan_sets(name, mode):
        assert ties.staged(name, mode, sname)
        _align(gpu_lib, name, mode, sname, 1)
    monkeypatch.setenv("GNX_WALK_LANE", "1")
    for sname in ties.plan_sets(name, mode):
        _align(gpu_lib, name, mode, sname, 1, what="one lane per pair")


@pytest.mark.parametrize("maxit", [None, "0", "3"])
def test_fast_path_checkerboard_and_rounds(gpu_lib, monkeypatch, maxit):
    """7 x 7 checkerboards inside the windows (Q1 on every seventh row of the re-filled windows), the windows re-filled in as many
    rounds as it takes, in none (every straggler through fill_affine) and in three"""
    monkeypatch.setenv("GNX_FASTPATH", "2")
    if maxit is not None:
        monkeypatch.setenv("GNX_FP_MAXIT", maxit)
    for sname in ties.plan_sets("fp2", 0):
        _align(gpu_lib, "fp2", 0, sname, None, ci=7, what="maxit %s" % maxit)


def test_fast_path_block_diag(gpu_lib, monkeypatch):
    """fp_walk's block_diag takes a whole row block in one stride when the plain diagonal scores what the handed-down rows say:
    "equality can only hold if h = M in every cell, and tripleMaxTrace gives such ties to M".  Three-block reads on a tandem repeat
    behind a unique head, with one indel of whole periods: anywhere in the repeat the indel costs the same, so at the M sites of
    the lower blocks M ties with the gap state, and the preference for M alone takes the indel up to the head -- inside the top block,
    where it keeps any whole-read diagonal from finishing the walk before block_diag is asked (ties.diag_condition: by the census and
    the oracle's CIGAR, in at least half of the pairs; tests/test_ties_cpu.py finds it in all twelve).  The batch runs under the tie
    table alone: it is about M against a gap state, a kernel that prefers D over I is the other batches' to find"""
    monkeypatch.setenv("GNX_FASTPATH", "2")
    assert len(ties.diag_condition()) >= 6
    _align(gpu_lib, "diag", 0, "tie15", 1)
    monkeypatch.setenv("GNX_WALK_LANE", "1")
    _align(gpu_lib, "diag", 0, "tie15", 1, what="one lane per pair")
