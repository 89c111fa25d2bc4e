"""gnx_md_* on the device against the literal restatement (tests/pyref_md.py): byte equality in both forms of the walk and across
sub-batch cuts, on the seams of the kernel, on every digit boundary of the decimals, on the device's own CIGARs and on the packed
resident reference; the reports with tags=True and the SAM lines they give; the error codes; the C++ mirror."""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

import md_cases as mc
import pyref_md as ref
import summary_cases as sc
import test_summary_gpu as tsg
from gonomics_amd import _lib, align, sam

pytestmark = pytest.mark.gpu

FORMS = [{}, {"GNX_MD_FORM": "0"}, {"GNX_MD_FORM": "1"}]
CUTS = [{}, {"GNX_MD_SUB": "1"}, {"GNX_MD_SUB": "3"}]
SWITCHES = [dict(f, **c) for f, c in itertools.product(FORMS, CUTS)]
SENTINEL = 0x5A5A5A5A


def _under(monkeypatch, env, call):
    for k in ("GNX_MD_FORM", "GNX_MD_SUB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return call()


def _params(mode):
    _, mx, go0, ge0 = sc.SCORING[0]
    go, ge = sc.pens(mode, go0, ge0)
    return _lib.make_params(mode, mx, go, ge)


def _device_md(p, alphas, betas, routes):
    ops, off = align._routes_to_ops(routes)
    return _lib.md_strings(*_lib.md_batch(p, alphas, betas, ops, off))


# ---- 1. seams: hand-made CIGARs, every form and cut ----
@pytest.mark.parametrize("mode", sc.MODES)
def test_seams(gpu_lib, monkeypatch, mode):
    cases = sc.seam_cases()
    p = _params(mode)
    alphas, betas, routes = [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]
    want = [ref.md(mode, a, b, r) for a, b, r in zip(alphas, betas, routes)]
    assert want[[c[0] for c in cases].index("m63_64_65")] == mc.M63_64_65
    for env in SWITCHES:
        got = _under(monkeypatch, env, lambda: _device_md(p, alphas, betas, routes))
        wrong = [(cases[k][0], got[k][:60], want[k][:60]) for k in range(len(cases)) if got[k] != want[k]]
        assert not wrong, (mode, env, wrong)
    t = _lib.get_timing()
    assert t["fast_path"] == 13 and t["cells"] == sum(r for route in routes for r, _ in route)
    # one pair alone, and the empty batch
    assert _device_md(p, alphas[:1], betas[:1], routes[:1]) == want[:1]
    md, off = _lib.md_batch(p, [], [], np.zeros(0, _lib.CIGAR_DTYPE), np.zeros(1, np.int64))
    assert md.shape[0] == 0 and off.tolist() == [0]


def test_worked_values_and_public_calls(gpu_lib):
    from gonomics_amd import dna
    alpha = dna.StringToBases(mc.ALPHA)
    for mode, beta, route, md in mc.WORKED:
        assert align.MDTags(_params(mode), [alpha], [dna.StringToBases(beta)], [[align.Cigar(*c) for c in route]]) == [md], (mode, beta)


# ---- 2. the decimals on every digit boundary; the long D group ----
@pytest.mark.parametrize("mode", [0, 3])
def test_digit_boundaries(gpu_lib, monkeypatch, mode):
    names, alphas, betas, routes = mc.batch_with([("digits",) + mc.digit_boundary()])
    want = [ref.md(mode, a, b, r) for a, b, r in zip(alphas, betas, routes)]
    k = names.index("digits")
    assert want[k] == mc.digit_boundary_md() and [int(x) for x in re.findall(r"[0-9]+", want[k])] == list(mc.STRETCHES)
    for env in FORMS + CUTS[1:]:
        assert _under(monkeypatch, env, lambda: _device_md(_params(mode), alphas, betas, routes)) == want, (mode, env)


@pytest.mark.parametrize("mode", [2, 3])
def test_d_group_across_a_block_of_runs(gpu_lib, monkeypatch, mode):
    names, alphas, betas, routes = mc.batch_with([("d_group",) + mc.d_group()])
    want = [ref.md(mode, a, b, r) for a, b, r in zip(alphas, betas, routes)]
    k = names.index("d_group")
    groups = re.findall(r"\^[A-Z]+", want[k])
    assert len(groups) == 1 and len(groups[0]) == 201 and len(routes[k]) > 64  # (one group of 200 letters out of 71 runs)
    for env in FORMS + CUTS[1:]:
        assert _under(monkeypatch, env, lambda: _device_md(_params(mode), alphas, betas, routes)) == want, (mode, env)


# ---- 3. the device's own CIGARs ----
@pytest.mark.parametrize("mode,checker", [(m, 10000) for m in sc.MODES] + [(0, 3), (1, 3)])  # (checkersize belongs to the low-memory modes)
def test_device_cigars(gpu_lib, monkeypatch, mode, checker):
    """Conditions on the inputs: a ^ group and a 0 between two events among the 200 pairs.  An empty MD ("0") cannot come out of
    related_pairs -- every sequence has a base, and every alignment of the library consumes its whole query -- so the batch gets a 201st
    pair with an empty sequence where the mode takes one (the high-memory modes; the low-memory ones refuse it with GNX_EEMPTY): an empty
    query in the mapping mode, an empty alpha elsewhere."""
    _, mx, go0, ge0 = sc.SCORING[0]
    go, ge = sc.pens(mode, go0, ge0)
    alphas, betas = [list(x) for x in sc.related_pairs(mode, 2000 + mode, 200, 60)]
    if mode in (2, 3, 4):
        empty, other = np.zeros(0, np.uint8), np.array([0, 1, 2, 3, 3], np.uint8)
        alphas.append(other if mode == sc.LOCAL else empty)
        betas.append(empty if mode == sc.LOCAL else other)
    p = _lib.make_params(mode, mx, go, ge, checker, checker)
    routes = [route for _, route in align.AlignBatch(p, alphas, betas)]
    want = [ref.md(mode, a, b, r) for a, b, r in zip(alphas, betas, routes)]
    assert any("^" in t for t in want[:200]) and any(re.search(r"[A-Z]0[\^A-Z]", t) for t in want[:200])
    assert mode in (0, 1) or want[200] == "0"
    for env in FORMS + CUTS[2:]:
        assert _under(monkeypatch, env, lambda: align.MDTags(p, alphas, betas, routes)) == want, (mode, checker, env)
    for text in want:
        assert ref.PATTERN.fullmatch(text)


# ---- 4. the resident reference, packed, with N exception blocks ----
def test_by_offset_equals_windows_on_the_unpacked_bytes(gpu_lib, monkeypatch):
    genome, windows = tsg._resident_cases()
    rng = np.random.default_rng(13)
    p = _params(sc.LOCAL)
    reads, routes = [], []
    for s, ln in windows:
        if ln >= 150:
            route = [(3, sc.D), (70, sc.M), (2, sc.I), (20, sc.M), (1, sc.D), (0, sc.M), (6, sc.D)]
            route[5] = (ln - sum(r for r, o in route if o in (sc.M, sc.D)), sc.M)
        else:
            route = [(ln, sc.M)]
        reads.append(tsg._read_for(rng, genome[s:s + ln], route, True))
        routes.append(route)
    ops, off = align._routes_to_ops(routes)
    r_cat, r_off = _lib._cat(reads)
    w_start, w_len = [w[0] for w in windows], [w[1] for w in windows]
    want = [ref.md(sc.LOCAL, genome[s:s + ln], reads[k], routes[k]) for k, (s, ln) in enumerate(windows)]
    assert sum(t.count("N") for t in want) > 0 and any("^" in t for t in want)  # (conditions on the inputs: N letters under substitutions)
    gpu_lib.set_reference(genome)
    try:
        for env in FORMS + CUTS[1:]:
            got = _under(monkeypatch, env, lambda: _lib.md_strings(*_lib.md_batch_by_offset(p, r_cat, r_off, w_start, w_len, ops, off)))
            exp = _lib.md_strings(*_lib.md_batch_windows(p, genome, w_start, w_len, r_cat, r_off[:-1], np.diff(r_off), ops, off))
            assert got == exp == want, env
        assert align.MDTagsByOffset(p, reads[:3], windows[:3], routes[:3]) == want[:3]
        bad = list(w_len)
        bad[-1] = 11  # a window beyond the reference
        with pytest.raises(_lib.GnxError) as ei:
            _lib.md_batch_by_offset(p, r_cat, r_off, w_start, bad, ops, off)
        assert ei.value.code == _lib.GNX_EINVAL
        with pytest.raises(_lib.GnxError) as ei:  # the window is the described side in the mapping mode only
            _lib.md_batch_by_offset(_params(2), r_cat, r_off, w_start, w_len, ops, off)
        assert ei.value.code == _lib.GNX_EINVAL
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 5. end to end: reports with tags, SAM lines ----
BASE_KEYS = {"best", "strand", "score", "window_start", "pos", "end", "route", "xcigar"} | set(_lib.SUMMARY_FIELDS)


def _check_tags(rep, read):
    if rep["best"] < 0:
        assert rep["md"] is None and rep["mapq"] == 0
        return
    t_len = sum(r for r, o in rep["route"] if o != sc.I)
    target = _lib.synthetic_reference_bases(rep["window_start"], t_len, tsg.SYN_SEED)
    query = tsg._rc(read) if rep["strand"] else read
    assert rep["md"] == ref.md(sc.LOCAL, target, query, [tuple(c) for c in rep["route"]])
    assert ref.parts(rep["md"]) == (rep["n_equal"], rep["n_mismatch"], rep["del_bases"])
    assert rep["mapq"] == ref.mapq(rep["score"], rep["second_score"]) and 0 <= rep["mapq"] <= 60


def _check_lines(lines, report):
    for line, rep in zip(lines, report):
        f = line.split("\t")
        if rep["best"] < 0:
            assert f[4] == "255" and not any(x.startswith("MD:Z:") for x in f)
            continue
        assert f[4] == str(rep["mapq"]) and 0 <= int(f[4]) <= 60
        assert f[12].startswith("NM:i:") and f[13] == "MD:Z:" + rep["md"]


def test_reports_with_tags(gpu_lib):
    reads = tsg._simulated_reads()
    mx, go, ge = align.DefaultScoreMatrix, -400, -30
    gpu_lib.check(gpu_lib.lib().gnx_set_reference_synthetic(tsg.SYN_LEN, tsg.SYN_SEED))
    try:
        gpu_lib.reference_index_build(tsg.K, 1)
        p = gpu_lib.make_params(sc.LOCAL, mx, go, ge)
        names = ["r%d" % r for r in range(64)]
        # single reads
        tuples = align.MapReads(p, reads, **tsg.VOTE)
        plain = align.MapReadsReport(p, reads, **tsg.VOTE)
        report = align.MapReadsReport(p, reads, tags=True, **tsg.VOTE)
        assert len(report) == 64 and all(set(d) == BASE_KEYS for d in plain)
        strands = set()
        for r, (rep, t) in enumerate(zip(report, tuples)):
            assert set(rep) == BASE_KEYS | {"md", "mapq", "second_score"} and {k: rep[k] for k in BASE_KEYS} == plain[r]
            others = [x for k, x in enumerate(t[4]) if k != t[0]]
            assert rep["second_score"] == (max(others) if others else None)
            _check_tags(rep, reads[r])
            if rep["best"] >= 0:
                strands.add(rep["strand"])
        assert strands == {0, 1} and any(d["second_score"] is not None for d in report) and any(d["best"] < 0 for d in report)  # (conditions on the inputs)
        assert any(re.search(r"[A-Z]", d["md"] or "") for d in report)
        _check_lines(sam.Lines(names, reads, report, "syn"), report)
        for ln, rep in zip(sam.Lines(names, reads, plain, "syn"), plain):  # without tags: today's lines
            assert ln.split("\t")[4] == "255" and "MD:Z:" not in ln
        # pairs
        plain = align.MapReadPairsReport(p, reads, 150, 600, 200, **tsg.VOTE)
        report = align.MapReadPairsReport(p, reads, 150, 600, 200, tags=True, **tsg.VOTE)
        pair_keys = BASE_KEYS | {"second_score", "proper", "tlen"}
        assert len(report) == 64 and all(set(d) == pair_keys for d in plain)
        strands = set()
        for r, rep in enumerate(report):
            assert set(rep) == pair_keys | {"md", "mapq"} and {k: rep[k] for k in pair_keys} == plain[r]
            _check_tags(rep, reads[r])
            if rep["best"] >= 0:
                strands.add(rep["strand"])
        assert strands == {0, 1}
        _check_lines(sam.Lines(names, reads, report, "syn", paired=True), report)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 6. errors: the stated code, both output pointers untouched ----
@pytest.mark.parametrize("what,code", [("op3", _lib.GNX_EINVAL), ("negative_run", _lib.GNX_EINVAL), ("too_much_alpha", _lib.GNX_EINVAL), ("too_much_beta", _lib.GNX_EINVAL),
                                       ("byte5_consumed", _lib.GNX_EBASE), ("byte5_in_the_unconsumed_tail", _lib.GNX_EBASE), ("good", _lib.GNX_OK)])
def test_errors_leave_the_outputs_untouched(gpu_lib, what, code):
    p = _params(_lib.GNX_AFFINE_GAP_HIGHMEM)
    alpha, beta = np.array([0, 1, 2, 3, 0, 1], np.uint8), np.array([0, 1, 2, 3, 0], np.uint8)
    route = {"op3": [(2, 0), (1, 3)], "negative_run": [(2, 0), (-1, 1)], "too_much_alpha": [(5, 0), (2, 2)], "too_much_beta": [(5, 0), (1, 1)]}.get(what, [(4, 0), (1, 2)])
    if what == "byte5_consumed":
        beta[1] = 5
    if what == "byte5_in_the_unconsumed_tail":
        alpha[5] = 7
    ops, off = align._routes_to_ops([route])
    a_cat, a_off = _lib._cat([alpha])
    b_cat, b_off = _lib._cat([beta])
    md, moff = ctypes.c_void_p(SENTINEL), ctypes.c_void_p(SENTINEL)
    rc = _lib.lib().gnx_md_batch(ctypes.byref(p), 1, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data, b_off.ctypes.data, ops.ctypes.data, off.ctypes.data,
                                 ctypes.byref(md), ctypes.byref(moff))
    assert rc == code, _lib.lib().gnx_last_error()
    if code == _lib.GNX_OK:
        assert md.value != SENTINEL and moff.value != SENTINEL
        _lib.lib().gnx_free(md)
        _lib.lib().gnx_free(moff)
    else:
        assert md.value == SENTINEL and moff.value == SENTINEL


# ---- 7. the C++ mirror ----
def test_cpp_md_mirror_runs(gpu_lib):
    import test_md_cpu
    test_md_cpu._build_cpp()
    assert subprocess.call([test_md_cpu.BIN]) == 0
