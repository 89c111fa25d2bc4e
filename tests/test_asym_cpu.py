"""The oracle may be trusted on an asymmetric score matrix: oracle/gnx_oracle.c is pinned by golden vectors made with symmetric tables
only, so its orientation -- scores[alpha base][beta base], align/affineGap.go:183, align/constGap.go:157, genomeGraph/search.go:246 --
is established here independently, on tests/asym.py's ASYM, against the pure-Python statements (pyref, py_gsw, pyref_span) and
through identities that hold only for the right orientation.  And every batch tests/test_asym_gpu.py runs is checked, on the oracle
alone, to tell ASYM from its transpose (or its complement image) in at least half of its pairs.  Runs on CPU."""
import numpy as np
import pytest

import asym
import common
import oracle
import pyref
import pyref_span
from asym import ASYM, ASYM_RC, ASYM_T, COMPLEMENT


def test_matrix_properties():
    flat = [v for row in ASYM for v in row]
    assert len(set(flat)) == 25
    assert all(abs(ASYM[a][b] - ASYM[b][a]) >= 4 for a in range(5) for b in range(5) if a != b)
    assert ASYM_T == [list(col) for col in zip(*ASYM)] and ASYM_T != ASYM
    assert ASYM_RC == [[ASYM[COMPLEMENT[a]][COMPLEMENT[b]] for b in range(5)] for a in range(5)]
    assert ASYM_RC != ASYM and ASYM_RC != ASYM_T
    assert ASYM[4] != [ASYM[a][4] for a in range(5)]  # the N row against the N column
    assert all(ASYM[a][a] != ASYM_RC[a][a] for a in range(4))  # a complemented table shows on exact matches already
    # no route is lost: s - 2 * gapExtend and 4 * (s - 2 * gapExtend) stay inside the int16 bounds of the fast path and the sweeps
    for go, ge in asym.AFFINE_PENS + [asym.CHEAP_GAPS]:
        assert all(-16000 <= v - 2 * ge <= 16000 and -32000 <= 4 * (v - 2 * ge) <= 32767 for v in flat)
    assert all(-16000 <= v - 2 * asym.CONST_GAP <= 16000 for v in flat)


# ---- the oracle against the pure-Python statements -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_pairs():
    return common.random_pairs(901, 200, 1, 40, 1, 40)


@pytest.mark.parametrize("go,ge", asym.AFFINE_PENS)
@pytest.mark.parametrize("cs", [3, 10000])
def test_oracle_vs_pyref_affine(small_pairs, go, ge, cs):
    for a, b in zip(*small_pairs):
        al, bl = a.tolist(), b.tolist()
        assert oracle.align_one(oracle.MODE_AFFINE, ASYM, go, ge, a, b, cs, cs) == pyref.affine(al, bl, ASYM, go, ge, cs, cs)
        if cs == 10000:  # the high-memory modes have no checkerboard
            assert oracle.align_one(oracle.MODE_AFFINE_HIGHMEM, ASYM, go, ge, a, b) == pyref.affine(al, bl, ASYM, go, ge)
            assert oracle.align_one(oracle.MODE_AFFINE_LOCAL, ASYM, go, ge, a, b) == pyref.affine(al, bl, ASYM, go, ge, free_end=True)


@pytest.mark.parametrize("cs", [3, 10000])
def test_oracle_vs_pyref_const(small_pairs, cs):
    g = asym.CONST_GAP
    for a, b in zip(*small_pairs):
        al, bl = a.tolist(), b.tolist()
        assert oracle.align_one(oracle.MODE_CONST, ASYM, g, 0, a, b, cs, cs) == pyref.const(al, bl, ASYM, g, cs, cs)
        if cs == 10000:
            assert oracle.align_one(oracle.MODE_CONST_HIGHMEM, ASYM, g, 0, a, b) == pyref.const(al, bl, ASYM, g)


def test_swapped_sides_under_the_transposed_table(small_pairs):
    """score(a, b, S) == score(b, a, S^T) in the global high-memory modes -- and not under S itself, on these pairs"""
    alphas, betas = small_pairs
    for mode, go, ge in [(2, -400, -30), (2, -600, -150), (4, asym.CONST_GAP, 0)]:
        fwd = oracle.align_batch(mode, ASYM, go, ge, alphas, betas)[0]
        assert np.array_equal(fwd, oracle.align_batch(mode, ASYM_T, go, ge, betas, alphas)[0])
        assert np.mean(fwd != oracle.align_batch(mode, ASYM, go, ge, betas, alphas)[0]) >= 0.5


@pytest.mark.parametrize("side", [0, 1])
def test_gsw_oracle_vs_independent_statement(side):
    from test_n2_gsw import _cases, py_gsw
    for alpha, beta in _cases(905 + side, 200, 60, 60):
        assert oracle.gsw_extend(side, ASYM, asym.GSW_GAP, alpha, beta) == py_gsw(side, alpha, beta, ASYM, asym.GSW_GAP)


def test_chunk_of_one_is_the_highmem_alignment(small_pairs):
    for go, ge in asym.AFFINE_PENS:
        for a, b in zip(small_pairs[0][:100], small_pairs[1][:100]):
            assert oracle.affine_gap_chunk(ASYM, go, ge, 1, a, b) == oracle.align_one(oracle.MODE_AFFINE_HIGHMEM, ASYM, go, ge, a, b)


@pytest.mark.parametrize("chunk", [1, 3])
def test_one_member_groups_are_the_chunk_alignment(chunk):
    alphas, betas = asym.chunk_pairs(chunk)
    for go, ge in asym.AFFINE_PENS:
        for a, b in zip(alphas[:12], betas[:12]):
            assert oracle.multiple_affine_gap(ASYM, go, ge, chunk, a[None, :], b[None, :]) == oracle.affine_gap_chunk(ASYM, go, ge, chunk, a, b)


def test_span_from_the_oracle_and_computed_directly():
    """pyref_span.spans_from_oracle reads start and end off the oracle's CIGAR; the same span comes out of pyref's own CIGAR and out of
    the scalar model of the stage-2 recurrence, which indexes the table itself (target base first)"""
    targets, queries = common.random_pairs(907, 40, 1, 150, 1, 90)
    for go, ge in asym.AFFINE_PENS:
        S, start, end = pyref_span.spans_from_oracle(ASYM, go, ge, targets, queries)
        for p, (t, q) in enumerate(zip(targets, queries)):
            score, route = pyref.affine(t.tolist(), q.tolist(), ASYM, go, ge, free_end=True)
            lead = route[0][0] if route[0][1] == 2 and len(route) > 1 else 0
            trail = route[-1][0] if route[-1][1] == 2 else 0
            assert (score, lead, len(t) - trail) == (int(S[p]), int(start[p]), int(end[p])), p
            for strip in (192, 7):
                got_start, got_score, _ = pyref_span.model_span(t, q, ASYM, go, ge, S[p], end[p], strip=strip)
                assert (got_score, got_start) == (int(S[p]), int(start[p])), (p, strip)


# ---- every batch of the GPU module tells the orientations apart (the oracle alone: no GPU needed) -------------------------------------
@pytest.mark.parametrize("name,modes", asym.ALIGN_BATCHES, ids=[b[0] for b in asym.ALIGN_BATCHES])
def test_align_batches_tell_orientation(name, modes):
    for mode in modes:
        for go, ge in asym.pens(mode):
            assert asym.tells(name, mode, go, ge)
            if mode < 2 and name in ("small", "long16", "fp2", "long40", "w64", "panels"):  # (run with small checkerboards as well)
                ci = {"small": 7, "long16": 7, "fp2": 7, "long40": 3, "w64": 16, "panels": 1000}[name]
                assert asym.tells(name, mode, go, ge, ci=ci)


def test_cheap_gap_batches_tell_orientation_and_overflow():
    for name, mode in (("fp_cheap", 0), ("xp_cheap", 3)):
        go, ge = asym.CHEAP_GAPS
        assert asym.tells(name, mode, go, ge)
        exp = asym.expected(name, mode, "ASYM", go, ge)
        runs = np.diff(exp[2])
        assert 1 <= int(np.sum(runs > 64)) <= len(runs) // 2, runs  # a few CIGARs beyond the 64 runs the fast path stages


def test_by_offset_batches_tell_orientation():
    ref, reads, w_start, w_len = asym.global_ref_batch()
    wins = [ref[s:s + l] for s, l in zip(w_start, w_len)]
    assert any(len(r) < len(w) for r, w in zip(reads, wins)) and any(len(r) > len(w) for r, w in zip(reads, wins))
    for mode in (0, 1, 2, 4):
        for go, ge in asym.pens(mode):
            asym.assert_tells_orientation(mode, go, ge, reads, wins)
    targets, queries = asym.batch("local")
    assert any(len(t) < len(q) for t, q in zip(targets, queries))
    assert any(len(q) <= 192 for q in queries) and any(len(q) > 192 for q in queries)


@pytest.mark.parametrize("chunk", [1, 3, 5])
def test_chunk_batches_tell_orientation(chunk):
    alphas, betas = asym.chunk_pairs(chunk)
    assert any(len(a) > len(b) for a, b in zip(alphas, betas)) and any(len(a) < len(b) for a, b in zip(alphas, betas))
    for go, ge in asym.AFFINE_PENS:
        asym.assert_tells_orientation(("chunk", chunk), go, ge, alphas, betas)


@pytest.mark.parametrize("chunk", [1, 2])
def test_group_batches_tell_orientation(chunk):
    blocks, pairs = asym.groups(chunk)
    assert sorted({b.shape[0] for b in blocks}) == [1, 2, 3, 4]
    for go, ge in asym.AFFINE_PENS:
        asym.assert_tells_orientation(("multi", chunk), go, ge, [blocks[x] for x, _ in pairs], [blocks[y] for _, y in pairs])


@pytest.mark.parametrize("side", [0, 1])
def test_gsw_batches_tell_orientation(side):
    pairs = asym.gsw_pairs(side)
    asym.assert_tells_orientation(("gsw", side), asym.GSW_GAP, 0, [a for a, _ in pairs], [b for _, b in pairs])


@pytest.mark.parametrize("mode", range(5))
def test_best_of_batch_tells_the_complemented_table(mode):
    from test_best_of_gpu import _flatten
    reads, target, cands = asym.best_of_workload()
    assert 35 <= len(reads) <= 45 and all(2 <= len(c) <= 4 for c in cands) and all(30 <= len(r) <= 200 for r in reads)
    alphas, betas = _flatten(mode, reads, target, cands)
    for go, ge in asym.pens(mode):
        asym.assert_tells_orientation(mode, go, ge, alphas, betas, other=ASYM_RC)
        asym.assert_tells_orientation(mode, go, ge, alphas, betas, other=ASYM_T)
