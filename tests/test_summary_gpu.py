"""gnx_summarize_* on the device against the literal restatement (tests/pyref_summary.py): every field and the extended CIGAR, in both
forms of the walk and across sub-batch cuts; the packed reference on either side; the ties to gnx_align_batch / gnx_locate_span_batch /
MapReads / MapReadPairs; the error codes; the C++ mirror."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import pyref_summary as ref
import summary_cases as sc
from gonomics_amd import _lib, align, dna

pytestmark = pytest.mark.gpu

SWITCHES = [{}, {"GNX_SUMMARY_FORM": "0"}, {"GNX_SUMMARY_FORM": "1"}, {"GNX_SUMMARY_SUB": "7"}]


def _route(ops):
    return [(int(r), int(o)) for r, o in zip(ops["run_length"], ops["op"])]


def _same(a, b):
    """(summaries, xops, xoff) equal field by field (the padding bytes of a copied CIGAR array are nobody's)"""
    return a[0].tobytes() == b[0].tobytes() and (a[1]["run_length"] == b[1]["run_length"]).all() and (a[1]["op"] == b[1]["op"]).all() and (a[2] == b[2]).all()


def _under(monkeypatch, env, call):
    for k in ("GNX_SUMMARY_FORM", "GNX_SUMMARY_SUB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return call()


def _check_against_pyref(mode, mx, go, ge, alphas, betas, routes, out, xops, xoff, what):
    for k, route in enumerate(routes):
        exp, ex = ref.summarize(mode, mx, go, ge, alphas[k], betas[k], route)
        got = {f: int(out[f][k]) for f in ref.FIELDS}
        assert got == exp, (what, k, got, exp)
        assert int(out["_reserved"][k]) == 0
        assert _route(xops[xoff[k]:xoff[k + 1]]) == ex, (what, k)


# ---- 1. fuzz: the device's own CIGARs ----
@pytest.mark.parametrize("mode,checker", [(m, 10000) for m in sc.MODES] + [(0, 3), (1, 3)])  # (checkersize belongs to the low-memory modes)
def test_fuzz_device_cigars(gpu_lib, monkeypatch, mode, checker):
    for name, mx, go0, ge0 in sc.SCORING:
        go, ge = sc.pens(mode, go0, ge0)
        alphas, betas = sc.related_pairs(mode, 1000 + mode, 40, 200)
        p = _lib.make_params(mode, mx, go, ge, checker, checker)
        scores, ops, off = _lib.align_batch(p, alphas, betas)
        routes = [_route(ops[off[k]:off[k + 1]]) for k in range(len(alphas))]
        runs = [_under(monkeypatch, env, lambda: _lib.summarize_batch(p, alphas, betas, ops, off, xcigar=True)) for env in SWITCHES]
        out, xops, xoff = runs[0]
        assert _lib.get_timing()["fast_path"] == 12
        for other in runs[1:]:
            assert _same(runs[0], other), (name, mode)
        _check_against_pyref(mode, mx, go, ge, alphas, betas, routes, out, xops, xoff, (name, mode, checker))
        pinned = 0
        for k in range(len(alphas)):
            if sc.score_is_pinned(mode, alphas[k], betas[k], checker, checker):
                assert int(out["rescore"][k]) == int(scores[k]), (name, mode, checker, k)
                assert (int(out["alpha_used"][k]), int(out["beta_used"][k])) == (len(alphas[k]), len(betas[k])), (name, mode, k)
                pinned += 1
        assert pinned == len(alphas) or checker == 3
        bare = _lib.summarize_batch(p, alphas, betas, ops, off)  # without an extended CIGAR: the same summaries, n_xops included
        assert bare[0].tobytes() == out.tobytes() and bare[1] is None


# ---- 2. seams: hand-made CIGARs ----
@pytest.mark.parametrize("mode", sc.MODES)
def test_seams(gpu_lib, monkeypatch, mode):
    cases = sc.seam_cases()
    name, mx, go0, ge0 = sc.SCORING[0]
    go, ge = sc.pens(mode, go0, ge0)
    p = _lib.make_params(mode, mx, go, ge)
    alphas, betas, routes = [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]
    ops, off = align._routes_to_ops(routes)
    first = None
    for env in SWITCHES:
        out, xops, xoff = _under(monkeypatch, env, lambda: _lib.summarize_batch(p, alphas, betas, ops, off, xcigar=True))
        _check_against_pyref(mode, mx, go, ge, alphas, betas, routes, out, xops, xoff, (mode, env, [c[0] for c in cases]))
        if first is None:
            first = out
        assert out.tobytes() == first.tobytes()
    t = _lib.get_timing()
    assert t["fast_path"] == 12 and t["cells"] == sum(r for route in routes for r, _ in route)
    # one pair alone, and the empty batch
    out, xops, xoff = _lib.summarize_batch(p, alphas[:1], betas[:1], ops[:off[1]], off[:2], xcigar=True)
    _check_against_pyref(mode, mx, go, ge, alphas[:1], betas[:1], routes[:1], out, xops, xoff, "single")
    out, xops, xoff = _lib.summarize_batch(p, [], [], ops[:0], off[:1], xcigar=True)
    assert out.shape[0] == 0 and xops.shape[0] == 0 and xoff.tolist() == [0]


def test_public_summarize_and_format(gpu_lib):
    a = dna.StringToBases("ACGTACGTAC")
    b = dna.StringToBases("ACGAACTAC")
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, align.HumanChimpTwoScoreMatrix, -600, -150)
    route = [align.Cigar(6, align.ColM), align.Cigar(1, align.ColD), align.Cigar(3, align.ColM)]
    (s,) = align.Summarize(p, [a], [b], [route], xcigar=True)
    exp, ex = ref.summarize(2, align.HumanChimpTwoScoreMatrix, -600, -150, a, b, route)
    assert {f: s[f] for f in ref.FIELDS} == exp and [tuple(c) for c in s["xcigar"]] == ex
    assert align.FormatXCigar(s["xcigar"]) == "3=1X2=1D3=" and align.FormatXCigar([]) == "*"
    assert "xcigar" not in align.Summarize(p, [a], [b], [route])[0]


# ---- 3. the resident reference, packed, on either side ----
@functools.lru_cache(maxsize=None)
def _resident_cases():
    """a 20 000-base reference with N runs across a 64-base block edge (60 .. 70) and across a flag-word edge (4 090 .. 4 100); windows of
    150 bases at every dword phase, over both N runs and at the last bases"""
    rng = np.random.default_rng(9)
    genome = rng.integers(0, 4, size=20000).astype(np.uint8)
    genome[60:70] = 4
    genome[4090:4100] = 4
    starts = list(range(18)) + [4000, 4033, 4090, 4095, 4096, 20000 - 150, 20000 - 151]
    return genome, [(s, 150) for s in starts] + [(20000 - 7, 7), (19990, 0)]


def _read_for(rng, window, route, window_is_alpha):
    """the other sequence of `route` against `window`: a copy on the M columns with a tenth of them substituted"""
    read, w = [], 0
    mine_only, theirs_only = (I, D) if window_is_alpha else (D, I)
    for r, o in route:
        for _ in range(r):
            if o == M:
                read.append(int(window[w]) if rng.random() < 0.9 else int(rng.integers(0, 5)))
                w += 1
            elif o == theirs_only:
                w += 1
            else:
                read.append(int(rng.integers(0, 4)))
    return np.asarray(read, dtype=np.uint8)


M, I, D = sc.M, sc.I, sc.D


@pytest.mark.parametrize("mode", [_lib.GNX_AFFINE_GAP_HIGHMEM, _lib.GNX_AFFINE_GAP_LOCAL, _lib.GNX_CONST_GAP], ids=["global_beta", "local_alpha", "const_beta"])
def test_by_offset_equals_windows_on_the_unpacked_bytes(gpu_lib, monkeypatch, mode):
    genome, windows = _resident_cases()
    rng = np.random.default_rng(10 + mode)
    local = mode == _lib.GNX_AFFINE_GAP_LOCAL
    go, ge = sc.pens(mode, -600, -150)
    p = _lib.make_params(mode, align.HumanChimpTwoScoreMatrix, go, ge)
    reads, routes = [], []
    for s, ln in windows:
        if ln >= 150:  # window-only columns are D where the window is alpha (local) and I where it is beta
            mine = D if local else I
            route = [(3, mine), (70, M), (2, I), (20, M), (1, D), (0, M), (6, mine)]
            route[5] = (ln - sum(r for r, o in route if o in (M, mine)), M)
        else:
            route = [(ln, M)]
        reads.append(_read_for(rng, genome[s:s + ln], route, local))
        routes.append(route)
    ops, off = align._routes_to_ops(routes)
    r_cat, r_off = _lib._cat(reads)
    w_start, w_len = [w[0] for w in windows], [w[1] for w in windows]
    gpu_lib.set_reference(genome)
    try:
        for env in SWITCHES:
            got = _under(monkeypatch, env, lambda: _lib.summarize_batch_by_offset(p, r_cat, r_off, w_start, w_len, ops, off, xcigar=True))
            if local:
                exp = _lib.summarize_batch_windows(p, genome, w_start, w_len, r_cat, r_off[:-1], np.diff(r_off), ops, off, xcigar=True)
            else:
                exp = _lib.summarize_batch_windows(p, r_cat, r_off[:-1], np.diff(r_off), genome, w_start, w_len, ops, off, xcigar=True)
            assert _same(got, exp), env
        wins = [genome[s:s + ln] for s, ln in windows]
        alphas, betas = (wins, reads) if local else (reads, wins)
        _check_against_pyref(mode, align.HumanChimpTwoScoreMatrix, go, ge, alphas, betas, routes, got[0], got[1], got[2], mode)
        assert int(got[0]["n_equal"].sum()) > 100 * len(windows) - 400  # (a condition on the inputs: the reads do resemble their windows)
        # the public call; a window beyond the reference
        pub = align.SummarizeByOffset(p, reads[:3], windows[:3], routes[:3], xcigar=True)
        assert [d["rescore"] for d in pub] == [int(v) for v in got[0]["rescore"][:3]]
        bad = list(w_len)
        bad[-1] = 11
        with pytest.raises(_lib.GnxError) as ei:
            _lib.summarize_batch_by_offset(p, r_cat, r_off, w_start, bad, ops, off)
        assert ei.value.code == _lib.GNX_EINVAL
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 4. cross-entry ----
def test_local_summary_agrees_with_locate_span(gpu_lib):
    name, mx, go, ge = sc.SCORING[0]
    targets, queries = sc.related_pairs(sc.LOCAL, 1003, 40, 200)
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
    scores, ops, off = _lib.align_batch(p, targets, queries)
    out, _, _ = _lib.summarize_batch(p, targets, queries, ops, off)
    s_score, s_start, s_end = _lib.locate_span_batch(p, targets, queries)
    assert (out["alpha_start"] == s_start).all() and (out["alpha_end"] == s_end).all()
    assert (out["rescore"] == s_score).all() and (out["rescore"] == scores).all()


SYN_LEN, SYN_SEED, K = 65536, 11, 16
VOTE = dict(max_occ=16, bin=32, pad=16, max_cand=4, min_votes=2)
COMPLEMENT = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def _rc(x):
    return COMPLEMENT[np.asarray(x, dtype=np.uint8)[::-1]]


@functools.lru_cache(maxsize=None)
def _simulated_reads():
    """32 pairs of 100-base mates from fragments of 250 .. 450 bases of the synthetic reference, with substitutions and now and then a
    deleted or an inserted base, the reverse mate first in every other pair; pairs 5 and 21 have a mate of random bases (no candidate)"""
    rng = np.random.default_rng(43)
    genome = _lib.synthetic_reference_bases(0, SYN_LEN, SYN_SEED)
    reads = []
    for k in range(32):
        frag = int(rng.integers(250, 451))
        o = int(rng.integers(0, SYN_LEN - frag))
        pieces = [genome[o:o + 100].copy(), genome[o + frag - 100:o + frag].copy()]
        for q, x in enumerate(pieces):
            for at in rng.choice(100, size=int(rng.integers(0, 4)), replace=False):
                x[at] = (x[at] + rng.integers(1, 4)) % 4
            if k % 4 == 1:
                pieces[q] = np.delete(x, 50)
            elif k % 4 == 2:
                pieces[q] = np.insert(x, 50, (x[50] + 1) % 4)
        if k in (5, 21):
            pieces[1] = rng.integers(0, 4, size=100).astype(np.uint8)
        mates = [pieces[0], _rc(pieces[1])]
        reads += mates[::-1] if k % 2 else mates
    return reads


def _check_report(rep, reads, params_tuple, best, score, route, window_start):
    """one report dict against the values of the tuple interface and the restatement on the host's copy of the synthetic reference"""
    mx, go, ge = params_tuple
    assert (rep["best"], rep["score"], [tuple(c) for c in rep["route"]], rep["window_start"]) == (best, score, [tuple(c) for c in route], window_start)
    if best < 0:
        assert rep["pos"] is None and rep["xcigar"] == [] and rep["n_equal"] == 0
        return 0
    t_len = sum(r for r, o in route if o != I)
    target = _lib.synthetic_reference_bases(window_start, t_len, SYN_SEED)
    query = _rc(reads) if rep["strand"] else reads
    exp, ex = ref.summarize(sc.LOCAL, mx, go, ge, target, query, route)
    assert {f: rep[f] for f in ref.FIELDS} == exp and [tuple(c) for c in rep["xcigar"]] == ex
    assert rep["rescore"] == score and rep["pos"] == window_start + exp["alpha_start"] and rep["end"] == window_start + exp["alpha_end"]
    return exp["n_mismatch"] + exp["ins_bases"] + exp["del_bases"]


def test_reports_agree_with_the_tuple_interfaces(gpu_lib):
    from gonomics_amd import sam
    reads = _simulated_reads()
    name, mx, go, ge = "Default", align.DefaultScoreMatrix, -400, -30
    gpu_lib.check(gpu_lib.lib().gnx_set_reference_synthetic(SYN_LEN, SYN_SEED))
    try:
        gpu_lib.reference_index_build(K, 1)
        p = gpu_lib.make_params(sc.LOCAL, mx, go, ge)
        # single reads
        tuples = align.MapReads(p, reads, **VOTE)
        report = align.MapReadsReport(p, reads, **VOTE)
        assert len(report) == len(tuples) == 64
        strands, edits = set(), 0
        for r, (rep, t) in enumerate(zip(report, tuples)):
            edits += _check_report(rep, reads[r], (mx, go, ge), t[0], t[1], t[2], t[5])
            if t[0] >= 0:
                assert rep["end"] == t[5] + t[3]
                strands.add(rep["strand"])
        assert strands == {0, 1} and edits > 0 and sum(1 for t in tuples if t[0] < 0) >= 2  # (conditions on the inputs)
        lines = sam.Lines(["r%d" % r for r in range(64)], reads, report, "syn")
        for r, line in enumerate(lines):
            f = line.split("\t")
            rep = report[r]
            if rep["best"] < 0:
                assert f[1:9] == ["4", "*", "0", "255", "*", "*", "0", "0"]
                continue
            assert f[1] == ("16" if rep["strand"] else "0") and f[2] == "syn" and int(f[3]) == rep["pos"] + 1
            assert "NM:i:%d" % (rep["n_mismatch"] + rep["ins_bases"] + rep["del_bases"]) in f and "AS:i:%d" % rep["score"] in f
            assert "D" not in (f[5][-1], f[5].lstrip("0123456789")[0])  # no free end gap in the SAM CIGAR
        # pairs
        per_read, per_pair = align.MapReadPairs(p, reads, 150, 600, 200, **VOTE)
        report = align.MapReadPairsReport(p, reads, 150, 600, 200, **VOTE)
        assert len(report) == 64 and sum(pr for pr, _ in per_pair) >= 16
        for r, (rep, t) in enumerate(zip(report, per_read)):
            w_start = None if t[0] < 0 else t[5] - (t[2][0][0] if len(t[2]) > 1 and t[2][0][1] == D else 0)
            _check_report(rep, reads[r], (mx, go, ge), t[0], t[1], t[2], w_start)
            assert (rep["pos"], rep["end"], rep["second_score"]) == (t[5], t[6], t[7])
            assert (rep["proper"], rep["tlen"]) == per_pair[r // 2]
        lines = sam.Lines(["r%d" % r for r in range(64)], reads, report, "syn", paired=True)
        for k, (proper, tlen) in enumerate(per_pair):
            f1, f2 = lines[2 * k].split("\t"), lines[2 * k + 1].split("\t")
            assert bool(int(f1[1]) & 2) == proper and bool(int(f2[1]) & 2) == proper
            assert sorted([int(f1[8]), int(f2[8])]) == ([-tlen, tlen] if proper else [0, 0])
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 5. errors: the stated code, nothing written ----
def _raw_call(p, alpha, beta, ops, ops_off, out):
    L = _lib.lib()
    a_cat, a_off = _lib._cat([alpha])
    b_cat, b_off = _lib._cat([beta])
    return L.gnx_summarize_batch(ctypes.byref(p), 1, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data, b_off.ctypes.data, ops.ctypes.data, ops_off.ctypes.data,
                                 out.ctypes.data, None, None)


@pytest.mark.parametrize("what,code", [("op3", _lib.GNX_EINVAL), ("negative_run", _lib.GNX_EINVAL), ("too_much_alpha", _lib.GNX_EINVAL), ("too_much_beta", _lib.GNX_EINVAL),
                                       ("byte5_consumed", _lib.GNX_EBASE), ("byte5_in_the_unconsumed_tail", _lib.GNX_EBASE), ("good", _lib.GNX_OK)])
def test_errors_leave_the_output_untouched(gpu_lib, what, code):
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, align.HumanChimpTwoScoreMatrix, -600, -150)
    alpha, beta = np.array([0, 1, 2, 3, 0, 1], np.uint8), np.array([0, 1, 2, 3, 0], np.uint8)
    route = {"op3": [(2, 0), (1, 3)], "negative_run": [(2, 0), (-1, 1)], "too_much_alpha": [(5, 0), (2, 2)], "too_much_beta": [(5, 0), (1, 1)]}.get(what, [(4, 0), (1, 2)])
    if what == "byte5_consumed":
        beta[1] = 5
    if what == "byte5_in_the_unconsumed_tail":
        alpha[5] = 7
    ops, off = align._routes_to_ops([route])
    out = np.full(12, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    assert _raw_call(p, alpha, beta, ops, off, out) == code, _lib.lib().gnx_last_error()
    assert (out == 0x5A5A5A5A5A5A5A5A).all() == (code != _lib.GNX_OK)


# ---- 6. the C++ mirror ----
def test_cpp_summary_mirror_runs(gpu_lib):
    import test_summary_cpu
    test_summary_cpu._build_cpp()
    assert subprocess.call([test_summary_cpu.BIN]) == 0
