"""Every kernel route at the edges of its numeric admission rule (tests/envelope.py has the rules and the cases; DESIGN.md "Numeric
envelope" the table).  Each rule's parameter sets -- the last value it admits at either end, the first it refuses -- run through every
route the rule governs, forced with the switches the other suites use and asserted through the timing's fast_path.  Every comparison
is equality with the oracle on the same inputs: score, offsets, every CIGAR run (common.assert_same); the score and locate entries
against the scores and ends derived from the oracle's alignment.  No tolerance anywhere; a route other than the expected one fails."""
import os

import numpy as np
import pytest

import common
import envelope as env
import envelope_oracle as envo
import oracle
import pyref_span

pytestmark = pytest.mark.gpu

ROUTE_SWITCHES = ("GNX_FASTPATH", "GNX_NO_HFORM", "GNX_LAT", "GNX_WIDE", "GNX_CLONG", "GNX_W64", "GNX_REBASE", "GNX_CL_CKC", "GNX_MEGA_STRIPS",
                  "GNX_W64_FARM", "GNX_W64_SPEC", "GNX_W64_CK", "GNX_W64_R", "GNX_W64_RC", "GNX_FP_MAXIT", "GNX_FP_CERT", "GNX_SCORE_SWEEP", "GNX_NO_PIPE",
                  "GNX_FORCE_P16", "GNX_CONST_P32", "GNX_CL_P16", "GNX_CL_WG", "GNX_SCORE_GENERIC")
GENERAL = {"GNX_FASTPATH": "0", "GNX_LAT": "0", "GNX_CLONG": "0"}
SNAP16 = {"GNX_CLONG": "2", "GNX_W64": "0"}
SNAP64 = {"GNX_CLONG": "2", "GNX_W64": "2"}


# Switches set from OUTSIDE (tools/switch_matrix.sh) stand wherever a case does not set the same switch itself: the results must not
# change, "which path ran" legitimately does -- then only the results are checked, as in the other suites.
OUTER = common.OUTER_ROUTE_SWITCH or any(k in os.environ for k in ROUTE_SWITCHES)  # (at import: before any monkeypatch)


class _Env:
    """switches for the length of a `with` block, on top of the test's monkeypatch"""

    def __init__(self, monkeypatch, switches):
        self.mp, self.sw = monkeypatch, switches

    def __enter__(self):
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()
        for k, v in self.sw.items():
            m.setenv(k, v)
        return m

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


def _params(L, c, ci=10000):
    return L.make_params(c.mode, c.scores, c.gap_open, c.gap_extend, ci, ci)


def _route_is(tm, route, what):
    """route: 0 / 1 / 2 through common.expect_route (3 counts as 0, 6 as 2), any other number or a tuple exactly; None: not asserted"""
    if route is None:
        return
    if OUTER:
        return
    if route in (0, 1, 2):
        common.expect_route(tm, route)
    else:
        assert tm["fast_path"] in (route if isinstance(route, tuple) else (route,)), (tm["fast_path"], route, what)


def _align(L, c, key, alphas, betas, route, ci=10000, what=""):
    """align_batch of a case on a batch under the switches in force: the oracle's bits and the route asked for"""
    got = L.align_batch(_params(L, c, ci), alphas, betas)
    tm = L.get_timing()
    common.assert_same(got, envo.expected(c, key, alphas, betas, ci), "%s | %s %s checkersize %d" % (c.label, key, what, ci))
    _route_is(tm, route, "%s | %s %s" % (c.label, key, what))
    return got


def _cases(rule, keep=lambda c: True):
    cs = [c for c in env.cases(rule) if keep(c)]
    return pytest.mark.parametrize("case", cs, ids=[c.label for c in cs])


# ---- K27: static int32 keys ---------------------------------------------------------------------------------------------------------
@_cases("K27", lambda c: not env.k27_is_fast_path_family(c))
def test_k27_static_keys(gpu_lib, monkeypatch, case):
    """(n + m + 2) * maxpen on either side of 2^27 with |score| = 2^20: pairs of 125 / 126 bases in all whose optimal scores reach
    +- 0.48 * 2^27 (and, at the largest score the 64-lane kernels take, pairs of 1 013 a side).  Admitted: the stored-matrix path, the latency geometry, the snapshot path on absolute keys (16 and 64 lanes).
    Refused: no switch -- the snapshot path on moving bases where there is one (routes 2 / 6), else the int64 kernel (4)."""
    alphas, betas = env.batch_total(case)
    assert all(env.k27(case.mode, case.scores, case.gap_open, case.gap_extend, len(a), len(b)) == case.admitted for a, b in zip(alphas, betas))
    if not case.admitted:
        _align(gpu_lib, case, "k27", alphas, betas, (2, 6, 4), what="default routing")
        return
    for ci in ((7, 10000) if case.mode in (0, 1) else (10000,)):
        with _Env(monkeypatch, GENERAL):
            _align(gpu_lib, case, "k27", alphas, betas, 0, ci, "general path")
        with _Env(monkeypatch, {"GNX_LAT": "2"}):
            _align(gpu_lib, case, "k27", alphas, betas, 3, ci, "latency geometry")
        if case.mode != env.LOCAL:
            with _Env(monkeypatch, SNAP16):
                _align(gpu_lib, case, "k27", alphas, betas, (2,), ci, "snapshot path, 16 lanes")
            with _Env(monkeypatch, SNAP64):  # (SPR bounds the 64-lane kernels on absolute keys too: |score| = 2^20 stays on 16 lanes)
                w64 = env.spr_w64(case.mode, case.scores, case.gap_open, case.gap_extend)
                assert w64 == (" w64 " in case.label)
                _align(gpu_lib, case, "k27", alphas, betas, 6 if w64 else (2,), ci, "snapshot path, 64 lanes")


@_cases("K27", env.k27_is_fast_path_family)
def test_k27_fast_path(gpu_lib, monkeypatch, case):
    """the same rule where FP16 admits the table too: reads of one and of several row blocks (AffineGapLocal: queries, the transposed
    form) against windows that take n + m + 2 to the last admitted total -- 1 242 with gap extensions of 50 000, whose trailing gap
    carries the keys to - 0.46 * 2^27; 16 170 and 5 592 with the profile's own extremes"""
    assert env.fp16(case.mode, case.scores, case.gap_open, case.gap_extend)
    for key, rows in (("k27", env.K27_FP_ROWS1), ("k27 blocks", env.K27_FP_ROWS23)):
        alphas, betas = env.batch_total(case, rows=rows)
        if not case.admitted:
            _align(gpu_lib, case, key, alphas, betas, (2, 6, 4), what="default routing")
            continue
        with _Env(monkeypatch, {"GNX_FASTPATH": "2"}):
            _align(gpu_lib, case, key, alphas, betas, 1, what="fast path")
        with _Env(monkeypatch, GENERAL):
            _align(gpu_lib, case, key, alphas, betas, 0, what="general path")


# ---- P26: the parameters the library takes at all -----------------------------------------------------------------------------------------
@_cases("P26")
def test_p26_parameter_range(gpu_lib, case):
    """|score|, |gapOpen|, |gapExtend| = 2^26: every pair is beyond every int32 route and runs the int64 kernel; 2^26 + 1: GNX_ERANGE"""
    alphas, betas = env.pairs(26, env.SHAPES["tiny"][:7], swap=(case.mode == env.LOCAL))
    if case.admitted:
        _align(gpu_lib, case, "p26", alphas, betas, 4)
        return
    for fn in (gpu_lib.align_batch, gpu_lib.score_batch):
        with pytest.raises(gpu_lib.GnxError) as ei:
            fn(_params(gpu_lib, case), alphas, betas)
        assert ei.value.code == gpu_lib.GNX_ERANGE, case.label


# ---- FP16: the fast path's int16 profile -------------------------------------------------------------------------------------------------
def _by_offset(L, c, alphas, betas):
    """the batch with its betas as windows of ONE packed resident reference"""
    ref = np.concatenate(betas)
    r_len = np.asarray([len(b) for b in betas], np.int64)
    r_start = np.concatenate([[0], np.cumsum(r_len)[:-1]]).astype(np.int64)
    a_off = np.concatenate([[0], np.cumsum([len(a) for a in alphas])]).astype(np.int64)
    L.set_reference(ref)
    try:
        got = L.align_batch_by_offset(_params(L, c), np.concatenate(alphas), a_off, r_start, r_len)
        return got, L.get_timing()
    finally:
        L.set_reference(np.zeros(0, np.uint8))


@_cases("FP16")
def test_fp16_fast_path_profile(gpu_lib, monkeypatch, case):
    """4 * (s - 2e) = 32 764 / - 32 000, gapOpen = - 7 999 / 0, the transposed form's gapExtend = - 7 999 / - 1 under GNX_FASTPATH=2:
    fp_sweep_kernel + fp_walk_kernel on one row block, the levels kernel on two and three, a window of the packed resident
    reference, the gapless certificate on and off, the tile re-fill for every walk; one step beyond: the general path"""
    monkeypatch.setenv("GNX_FASTPATH", "2")
    route = 1 if case.admitted else 0
    one, more = ("fp1 level", "fp23 level") if case.gap_open >= 0 else ("fp1", "fp23")  # (gapOpen = 0: see envelope.SHAPES)
    for name in (one, more):
        alphas, betas = env.batch_for(case, name)
        _align(gpu_lib, case, name, alphas, betas, route)
    if not case.admitted:
        return
    alphas, betas = env.batch_for(case, one)
    exp = envo.expected(case, one, alphas, betas)
    if case.mode != env.LOCAL:
        got, tm = _by_offset(gpu_lib, case, alphas, betas)
        common.assert_same(got, exp, case.label + " | windows of the resident reference")
        _route_is(tm, 1, case.label)
        res = {}
        for cert in ("2", "0"):
            with _Env(monkeypatch, {"GNX_FP_CERT": cert}):
                res[cert] = _align(gpu_lib, case, one, alphas, betas, 1, what="GNX_FP_CERT=" + cert)
        common.assert_same(res["2"], res["0"], case.label + " | certificate on and off")
    with _Env(monkeypatch, {"GNX_FP_MAXIT": "0"}):
        for name in (one, more):
            a2, b2 = env.batch_for(case, name)
            _align(gpu_lib, case, name, a2, b2, 1, what="GNX_FP_MAXIT=0")
        if case.mode in (0, 1):
            _align(gpu_lib, case, one, alphas, betas, None, ci=7, what="GNX_FP_MAXIT=0")


# ---- SN16: the snapshot path's int16 profile ----------------------------------------------------------------------------------------------
@_cases("SN16")
def test_sn16_snapshot_profile(gpu_lib, monkeypatch, case):
    """4 * (s - 2g) + 1 = 32 765 / - 32 767 and one step beyond, through the 16-lane kernels, the 64-lane kernels (and their farm:
    pairs of two 640-row strips), and row panels of three 160-row / two 640-row strips; an admitted set again with the int32 profile (GNX_CL_P16=0)"""
    lowmem = case.mode in (0, 1)
    legs = [("snap", SNAP16, (2,), "16 lanes"), ("snap", SNAP64, 6, "64 lanes"), ("farm", SNAP64, 6, "64 lanes, farm"),
            ("panels", {"GNX_MEGA_STRIPS": "3"}, 5, "row panels"), ("farm", {"GNX_MEGA_STRIPS": "2", "GNX_W64": "2"}, 5, "row panels, 64 lanes")]
    for name, sw, route, what in legs:
        alphas, betas = env.batch_for(case, name)
        with _Env(monkeypatch, sw):
            got = _align(gpu_lib, case, name, alphas, betas, route, what=what)
            if lowmem and name == "snap":
                _align(gpu_lib, case, name, alphas, betas, route, ci=16, what=what)
        if case.admitted and "GNX_CLONG" in sw:
            with _Env(monkeypatch, dict(sw, GNX_CL_P16="0")):
                again = _align(gpu_lib, case, name, alphas, betas, route, what=what + ", GNX_CL_P16=0")
            common.assert_same(got, again, case.label + " | int16 and int32 profile, " + what)


# ---- GP16 / CP16: the general path's int16 profiles ------------------------------------------------------------------------------------------
@_cases("GP16")
def test_gp16_general_path_affine_profile(gpu_lib, monkeypatch, case):
    """fill_affine_kernel<.., P16> (GNX_FORCE_P16=1; the library's own choice is the int32 profile) at 4 * (s - 2e) = 32 764 / - 32 768:
    one strip, several strips on one wave, piped strips; global and local; with the rebased tables, and with the plain ones
    (GNX_NO_HFORM, gapOpen > 0), whose entries are 4 * s: - 32 768 at their lower end"""
    base = dict(GENERAL, **({"GNX_NO_HFORM": "1"} if env.gp16_is_plain(case) else {}))
    for name in ("strip", "multi", "piped"):
        alphas, betas = env.batch_for(case, name)
        for force in (True, False):
            sw = dict(base, **({"GNX_FORCE_P16": "1"} if force else {}))
            with _Env(monkeypatch, sw):
                _align(gpu_lib, case, name, alphas, betas, 0, what="GNX_FORCE_P16 %s" % force)
                if case.mode == 0 and name != "piped":
                    _align(gpu_lib, case, name, alphas, betas, 0, ci=7, what="GNX_FORCE_P16 %s" % force)
            if force and name == "strip":
                with _Env(monkeypatch, dict(sw, GNX_NO_HFORM="1")):
                    _align(gpu_lib, case, name, alphas, betas, 0, what="GNX_FORCE_P16, GNX_NO_HFORM")


@_cases("CP16")
def test_cp16_general_path_const_profile(gpu_lib, monkeypatch, case):
    """piped fill_const_kernel<.., P16> at 4 * (s - 2 gap) + 1 = 32 765 / - 32 767 and with the int32 profile (GNX_CONST_P32=1); the
    single-wave forms, which always keep int32, on the same tables"""
    for name in ("piped", "multi", "strip"):
        alphas, betas = env.batch_for(case, name)
        for p32 in (False, True):
            with _Env(monkeypatch, dict(GENERAL, **({"GNX_CONST_P32": "1"} if p32 else {}))):
                _align(gpu_lib, case, name, alphas, betas, 0, what="GNX_CONST_P32 %s" % p32)
                if case.mode == 1 and name == "piped":
                    _align(gpu_lib, case, name, alphas, betas, 0, ci=7, what="GNX_CONST_P32 %s" % p32)


# ---- SS: the score sweeps -----------------------------------------------------------------------------------------------------------------
def _chunk_scores(c, alphas, betas):
    return [oracle.affine_gap_chunk(c.scores, c.gap_open, c.gap_extend, 1, a, b)[0] for a, b in zip(alphas, betas)]


@_cases("SS")
def test_ss_score_sweeps(gpu_lib, case):
    """score_batch (route 7; 8 for AffineGapLocal), locate_batch (8), locate_span_batch (10) and the chunk score entry (9) at
    s - 2 * reb = +- 16 000, gapOpen = - 16 000 / 0, gapExtend = - 8 000 / 0 and at the last total the rebased keys admit -- whose gap
    runs carry them to - 0.5 * 2^29 -- and one step beyond each, where the ordinary routes answer"""
    keys = env.ss_is_key_family(case)
    if keys:
        alphas, betas = env.batch_total(case, rows=env.ss_key_rows(case.mode))
        key = "sskeys"
        assert all(env.ss_keys(case.mode, case.scores, case.gap_open, case.gap_extend, len(a), len(b)) == case.admitted for a, b in zip(alphas, betas))
    else:
        alphas, betas = env.batch_for(case, "sweep")
        key = "sweep"
    p = _params(gpu_lib, case)
    swept = (7, 8, 9, 10)

    def route_ok(route, what):
        fp = gpu_lib.get_timing()["fast_path"]
        assert OUTER or ((fp == route) if case.admitted else (fp not in swept)), (case.label, what, fp)

    if case.mode == env.LOCAL:
        S, start, end = pyref_span.spans_from_oracle(case.scores, case.gap_open, case.gap_extend, alphas, betas, threads=8)
        for what, route, fn in (("score_batch", 8, gpu_lib.score_batch), ("locate_batch", 8, gpu_lib.locate_batch), ("locate_span_batch", 10, gpu_lib.locate_span_batch)):
            out = fn(p, alphas, betas)
            route_ok(route, what)  # (gapExtend = 0 too: the span kernel then takes the whole target as its window)
            out = (out,) if what == "score_batch" else out
            assert np.array_equal(out[0], S), (case.label, what, "score", np.flatnonzero(out[0] != S)[:8])
            if what != "score_batch":
                assert np.array_equal(out[-1], end), (case.label, what, "end", np.flatnonzero(out[-1] != end)[:8])
            if what == "locate_span_batch":
                assert np.array_equal(out[1], start), (case.label, what, "start", np.flatnonzero(out[1] != start)[:8])
        return
    exp = np.asarray(envo.expected(case, key, alphas, betas)[0], dtype=np.int64)
    got = gpu_lib.score_batch(p, alphas, betas)
    route_ok(7, "score_batch")
    assert np.array_equal(got, exp), (case.label, np.flatnonzero(got != exp)[:8], got[:4], exp[:4])
    if case.mode == 2:  # the chunk entry has AffineGap_highMem semantics; its sweep also needs the pairs inside K27 (the plain matrices of the other routes)
        got = gpu_lib.affine_gap_chunk_score_batch(p, 1, alphas, betas)
        fp = gpu_lib.get_timing()["fast_path"]
        inside = all(env.k27(case.mode, case.scores, case.gap_open, case.gap_extend, len(a), len(b)) for a, b in zip(alphas, betas))
        if not OUTER:
            assert (fp == 9) == (case.admitted and inside), (case.label, fp)
        assert [int(x) for x in got] == _chunk_scores(case, alphas, betas), case.label


# ---- N1: the chunk driver's int16 score matrix ------------------------------------------------------------------------------------------------
def _n1_got(sc, ops, off, k):
    return (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])


@_cases("N1")
def test_n1_chunk_score_matrix(gpu_lib, monkeypatch, case):
    """AffineGapChunk and multipleAffineGap with chunkSize 1 and 3 at 4 * chunk * max|s| + 8 * |e| * chunk = the last value an int16
    matrix holds and the first it does not: align calls in the latency geometry and on the general path, and their score twins"""
    chunk = case.chunk
    p = _params(gpu_lib, case)
    alphas, betas = env.n1_pairs(chunk)
    exp = [oracle.affine_gap_chunk(case.scores, case.gap_open, case.gap_extend, chunk, a, b) for a, b in zip(alphas, betas)]
    blocks, bpairs = env.n1_groups(chunk)
    gexp = [oracle.multiple_affine_gap(case.scores, case.gap_open, case.gap_extend, chunk, blocks[x], blocks[y]) for x, y in bpairs]
    for geometry in ("general", "lat"):
        if geometry == "lat":
            monkeypatch.delenv("GNX_FP_SMALL", raising=False)  # the shipped routing: small batches in the latency geometry
        else:
            monkeypatch.setenv("GNX_FP_SMALL", "1")
            monkeypatch.setenv("GNX_LAT", "0")
        sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
        for k in range(len(alphas)):
            assert _n1_got(sc, ops, off, k) == exp[k], (case.label, geometry, k)
        sc, ops, off = gpu_lib.multiple_affine_gap_batch(p, chunk, blocks, bpairs)
        for k in range(len(bpairs)):
            assert _n1_got(sc, ops, off, k) == gexp[k], (case.label, geometry, bpairs[k])
        monkeypatch.delenv("GNX_LAT", raising=False)
    got = gpu_lib.affine_gap_chunk_score_batch(p, chunk, alphas, betas)
    assert OUTER or gpu_lib.get_timing()["fast_path"] == 9
    assert [int(x) for x in got] == [e[0] for e in exp], case.label
    got = gpu_lib.multiple_affine_gap_score_batch(p, chunk, blocks, bpairs)
    assert OUTER or gpu_lib.get_timing()["fast_path"] == 9
    assert [int(x) for x in got] == [e[0] for e in gexp], case.label


# ---- SPR: the spread of the keys around a moving base ------------------------------------------------------------------------------------------
@_cases("SPR")
def test_spr_moving_bases(gpu_lib, monkeypatch, case):
    """GNX_CLONG=2 + GNX_REBASE=1 with step4 on either side of each threshold: the 64-lane affine sweep's snapshot spacing (2 048 / 1 024
    in row panels, 512 / 256 / 128 without, read back through gnx_debug_counter(6)), the 64-lane kernels at all (else the 16-lane ones), moving bases at all (else
    absolute keys for the pairs K27 admits -- and the int64 kernel for a pair that is really out of range)"""
    mode, sc, go, ge = case.mode, case.scores, case.gap_open, case.gap_extend
    monkeypatch.setenv("GNX_CLONG", "2")
    monkeypatch.setenv("GNX_REBASE", "1")
    if case.rule.startswith("SPRM"):  # row panels of two 640-row strips, always on moving bases
        for k, v in (("GNX_MEGA_STRIPS", "2"), ("GNX_W64", "2"), ("GNX_W64_R", "10")):
            monkeypatch.setenv(k, v)
        alphas, betas = env.batch_for(case, "farm")
        _align(gpu_lib, case, "farm", alphas, betas, 5)
        if not OUTER:
            assert gpu_lib.debug_counter(6, reset=False) == env.spr_mega_ck(mode, sc, go, ge), case.label
        return
    if case.rule != "SPR":  # the 64-lane legs
        monkeypatch.setenv("GNX_W64", "2")
        w64 = env.spr_w64(mode, sc, go, ge)
        assert w64 == (case.admitted or case.rule != "SPR64")
        alphas, betas = env.batch_for(case, "farm")
        _align(gpu_lib, case, "farm", alphas, betas, 6 if w64 else (2,))
        if w64 and not OUTER:
            assert gpu_lib.debug_counter(6, reset=False) == env.spr_w64_ck(mode, sc, go, ge), case.label
        return
    monkeypatch.setenv("GNX_W64", "0")
    alphas, betas = env.batch_for(case, "snap")
    inside = [k for k, (a, b) in enumerate(zip(alphas, betas)) if env.k27(mode, sc, go, ge, len(a), len(b))]
    assert 3 <= len(inside) < len(alphas)
    if case.admitted:  # moving bases: the pairs beyond K27 among them
        _align(gpu_lib, case, "snap", alphas, betas, 2)
        return
    _align(gpu_lib, case, "snap inside", [alphas[k] for k in inside], [betas[k] for k in inside], 2, what="absolute keys")
    monkeypatch.delenv("GNX_CLONG")
    monkeypatch.delenv("GNX_REBASE")
    monkeypatch.delenv("GNX_W64")
    _align(gpu_lib, case, "snap", alphas, betas, 4, what="beyond K27, no moving bases: the int64 kernel")


# ---- signs ---------------------------------------------------------------------------------------------------------------------------------
_SIGN_GROUPS = sorted(set(c.label.rsplit(" m", 1)[0] for c in env.sign_cases()))


@pytest.mark.parametrize("group", _SIGN_GROUPS)
def test_sign_family(gpu_lib, monkeypatch, group):
    """gapOpen = 0 and > 0, gapExtend = 0 and > 0, an all-positive and an all-zero table, at ordinary magnitudes and at 2^20, through
    the library's own routing and through the int64 kernel (GNX_WIDE=2): the oracle's bits.  No set here is one the library may
    refuse: an error code fails the test like a wrong answer"""
    for case in [c for c in env.sign_cases() if c.label.rsplit(" m", 1)[0] == group]:
        # every set is inside P26, every pair (n + m + 2 <= 127, |penalty| <= 2^20) inside K27: the library has to answer all of them
        assert env.p26(case.mode, case.scores, case.gap_open, case.gap_extend)
        alphas, betas = env.pairs(40, env.SHAPES["tiny"], swap=(case.mode == env.LOCAL))
        assert all(env.k27(case.mode, case.scores, case.gap_open, case.gap_extend, len(a), len(b)) for a, b in zip(alphas, betas))
        for sw in ({}, {"GNX_WIDE": "2"}):
            with _Env(monkeypatch, sw):
                _align(gpu_lib, case, "sign", alphas, betas, None, what=str(sw))
