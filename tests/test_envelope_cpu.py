"""tests/envelope.py checked without a GPU: every parameter set sits where its label says (on the last admitted value of its rule,
or one step beyond it), the two CPU statements of the path agree at these magnitudes, the key-range families really carry a pair to
the far end of the range ("teeth"), and in the int16 families the extreme entry of the table lies under an optimal path."""
import numpy as np
import pytest

import envelope as env
import envelope_oracle as envo
import oracle
import pyref

ALL_RULES = sorted(env.BUILDERS)
INT16_RULES = ("FP16", "SN16", "GP16", "CP16", "SS", "N1")


# ---- placement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ALL_RULES)
def test_every_set_sits_where_it_claims(rule):
    cs = env.cases(rule)
    assert len(set(c.label for c in cs)) == len(cs)
    assert any(c.admitted for c in cs) and any(not c.admitted for c in cs)
    for c in cs:
        assert env.admitted(c) == c.admitted, c.label
        if not c.admitted and c.undo is not None:  # one step back: admitted again
            assert env.admitted(env.stepped(c, c.undo)), c.label
        if c.admitted and c.extreme in ("hi", "both"):
            assert not env.admitted(env.stepped(c, ("score", env.A, env.A, 1))), c.label
        if c.admitted and c.extreme in ("lo", "both"):
            for a, b in env.LO_CELLS:
                assert not env.admitted(env.stepped(c, ("score", a, b, -1))), (c.label, a, b)
        if c.admitted and c.total is not None:
            assert not env.admitted(env.stepped(c, ("total", 1))) or "2^27//maxpen" in c.label, c.label
        assert (c.gap_extend == 0) or env.affine(c.mode)


@pytest.mark.parametrize("rule", ALL_RULES)
def test_tables_put_the_extremes_on_cells_the_inputs_use(rule):
    """the maximum on A/A, the minimum on A/C and N/G, and a table that differs from its transpose"""
    for c in env.cases(rule):
        f = env.flat(c.scores)
        sc = c.scores
        if c.extreme in ("hi", "both"):
            assert sc[env.A][env.A] == max(f), c.label
        if c.extreme in ("lo", "both") and c.undo is None:
            assert all(sc[a][b] == min(f) for a, b in env.LO_CELLS), c.label
        assert sum(1 for a in range(5) for b in range(a) if sc[a][b] != sc[b][a]) >= 8, c.label


def test_the_controlling_expressions_are_the_extreme_ones():
    """spelled out for one set per rule: the value the rule bounds equals its last admitted value"""
    c = env.by_label("FP16", "FP16 m0 e-150 last")
    assert 4 * (c.scores[0][0] - 2 * c.gap_extend) == 32764 and 4 * (c.scores[0][1] - 2 * c.gap_extend) == -32000 and c.gap_open == -7999
    c = env.by_label("SN16", "SN16 m0 hi last")
    assert 4 * (c.scores[0][0] - 2 * c.gap_extend) + 1 == 32765
    c = env.by_label("SN16", "SN16 m1 lo last")
    assert 4 * (c.scores[0][1] - 2 * c.gap_open) + 1 == -32767
    c = env.by_label("GP16", "GP16 m0 lo last")
    assert 4 * (c.scores[4][2] - 2 * c.gap_extend) == -32768
    c = env.by_label("CP16", "CP16 m4 hi last")
    assert 4 * (c.scores[0][0] - 2 * c.gap_open) + 1 == 32765
    c = env.by_label("SS", "SS m0 lo last")
    assert c.scores[0][1] - 2 * c.gap_extend == -16000 and c.gap_open == -16000
    c = env.by_label("N1", "N1 chunk 3 hi last")
    assert 4 * 3 * c.scores[0][0] + 8 * 30 * 3 == 32760 and 4 * 3 * (c.scores[0][0] + 1) + 8 * 30 * 3 > 32767
    c = env.by_label("K27", "K27 m0 pos last")
    assert c.total == 127 and c.total * (1 << 20) == (1 << 27) - (1 << 20)
    for rule, width in env.SPR_WIDTHS:
        c = env.by_label("SPR", "%s m0 last" % rule)
        s4 = env.step4(c.mode, c.scores, c.gap_open, c.gap_extend)
        assert width * s4 < (1 << 28) <= width * (s4 + 4)
    assert env.spr_mega_ck(0, env.by_label("SPR", "SPRM2048 m0 last").scores, -600, -150) == 2048
    assert env.spr_mega_ck(0, env.by_label("SPR", "SPRM2048 m0 first refused").scores, -600, -150) == 1024
    assert env.spr_mega_ck(0, env.by_label("SPR", "SPRM1024 m0 first refused").scores, -600, -150) == 512
    assert env.spr_w64_ck(0, env.by_label("SPR", "SPR512 m0 last").scores, -600, -150) == 512
    assert env.spr_w64_ck(0, env.by_label("SPR", "SPR512 m0 first refused").scores, -600, -150) == 256
    assert env.spr_w64_ck(0, env.by_label("SPR", "SPR256 m0 first refused").scores, -600, -150) == 128
    c = env.by_label("P26", "P26 m0 last")
    assert c.scores[0][0] == 1 << 26 and c.scores[0][1] == -(1 << 26) and c.gap_open == -(1 << 26)


def test_sequence_builder():
    al, be = env.pairs(5, env.SHAPES["tiny"])
    assert [(len(a), len(b)) for a, b in zip(al, be)] == env.SHAPES["tiny"]
    assert set(al[0]) == {env.A} == set(be[0]) and set(al[1]) == {env.A} and set(be[1]) == {env.C}
    assert not set(al[2]) & set(be[2]) and len(al[2]) != len(be[2])
    assert len(al[3]) * 4 <= len(be[3]) and len(al[5]) > 20 and np.sum((al[5][:50] == env.A) & (be[5][:50] == env.C)) >= 5
    assert np.sum(al[4] == env.N) >= 3 and np.any((al[4][:60] == env.N) & (be[4][:60] == env.G))
    for name, shapes in env.SHAPES.items():
        assert len(shapes) >= 6 and shapes[2][0] != shapes[2][1], name
    # the shapes are the smallest their route takes: piped strips, strips on one wave, the farm, one / two and three row blocks
    assert all(n > env.H16 and m >= 8 * env.RB_PUB for n, m in env.SHAPES["piped"]) and all(m < 8 * env.RB_PUB for n, m in env.SHAPES["multi"])
    assert all(n >= 2 * env.H64 for n, m in env.SHAPES["farm"]) and all(n > env.H16 for n, m in env.SHAPES["snap"])
    assert all(n <= env.H16 for n, m in env.SHAPES["fp1"]) and all(env.H16 < n <= 3 * env.H16 for n, m in env.SHAPES["fp23"])
    tl, tq = env.pairs(5, env.SHAPES["tiny"], swap=True)
    assert [(len(b), len(a)) for a, b in zip(tl, tq)] == env.SHAPES["tiny"] and set(tl[1]) == {env.A} and set(tq[1]) == {env.C}
    for total in (127, 128, 16390):
        assert all(n + m + 2 == total and n >= 1 and m >= 1 for n, m in env.split_total(total))


# ---- the reference at these magnitudes -----------------------------------------------------------------------------------------------
PYREF_SHAPES = [(30, 30), (29, 29), (20, 37), (10, 50), (31, 28), (1, 40)]


def _pyref(c, a, b, cs):
    al, bl = a.tolist(), b.tolist()
    if c.mode in env.CONST_MODES:
        return pyref.const(al, bl, c.scores, c.gap_open, *((cs, cs) if c.mode == 1 else ()))
    if c.mode == env.LOCAL:
        return pyref.affine(al, bl, c.scores, c.gap_open, c.gap_extend, free_end=True)
    return pyref.affine(al, bl, c.scores, c.gap_open, c.gap_extend, *((cs, cs) if c.mode == 0 else ()))


def _same_as_pyref(c, alphas, betas):
    for cs in ((7, 10000) if c.mode in (0, 1) else (10000,)):
        sc, ops, off = oracle.align_batch(c.mode, c.scores, c.gap_open, c.gap_extend, alphas, betas, cs, cs, threads=4)
        for k, (a, b) in enumerate(zip(alphas, betas)):
            got = (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])
            assert got == _pyref(c, a, b, cs), (c.label, k, cs)


@pytest.mark.parametrize("rule", ALL_RULES + ["SIGN"])
def test_oracle_equals_pyref_at_these_magnitudes(rule):
    """oracle.align_batch == pyref in score and CIGAR, checkerboards of 7 and 10 000, on every admitted set (the first refused ones
    differ from them by one unit) -- for K27 on the pairs of the GPU test itself, whose keys reach +- 2^27 / 2"""
    cs = env.sign_cases() if rule == "SIGN" else [c for c in env.cases(rule) if c.admitted or rule in ("K27", "P26")]
    for c in cs:
        if rule == "K27" and c.total <= 200:
            alphas, betas = env.batch_total(c)
        else:
            alphas, betas = env.pairs(31, PYREF_SHAPES, swap=(c.mode == env.LOCAL))
        _same_as_pyref(c, alphas, betas)


# ---- teeth --------------------------------------------------------------------------------------------------------------------------
def _k27_batch(c):
    if env.k27_is_fast_path_family(c):
        return env.batch_total(c, rows=env.K27_FP_ROWS1)
    return env.batch_total(c)


@pytest.mark.parametrize("case", [c for c in env.cases("K27") if not env.k27_is_fast_path_family(c) or " fp gaps " in c.label], ids=lambda c: c.label)
def test_k27_families_reach_the_end_of_the_key_range(case):
    """a condition on the inputs: some pair's optimal score is at least 0.45 * 2^27 in size -- 4 * score then passes 0.9 * 2^29.
    Of the families that FP16 admits too, the one with gap extensions of 50 000 has it (a trailing gap of 1 238 bases); the other two
    cannot: FP16 keeps their scores inside +- 8 191 + 2e and AffineGapLocal's gapExtend above - 8 000, so that no pair inside K27
    and inside the cells a test may spend gets beyond a third of the range.  They put the profile's extremes at the rule's last total."""
    alphas, betas = _k27_batch(case)
    sc = np.abs(envo.expected(case, "k27", alphas, betas)[0])
    assert int(sc.max()) >= 0.45 * (1 << 27), (case.label, int(sc.max()))


@pytest.mark.parametrize("case", [c for c in env.cases("SS") if env.ss_is_key_family(c) and c.mode != env.LOCAL], ids=lambda c: c.label)
def test_ss_key_families_reach_the_end_of_the_key_range(case):
    """some pair's optimal score is at least 0.45 * 2^29 / 2 in size.  (AffineGapLocal is left out by arithmetic: inserting the whole
    query costs at most 16 000 + 8 000 * 10 240 < 0.45 * 2^28, and a score above it needs 7 550 matches of 16 000 on both sides:
    more cells than a test here may spend.)"""
    alphas, betas = env.batch_total(case, rows=env.ss_key_rows(case.mode))
    sc = np.abs(envo.expected(case, "sskeys", alphas, betas)[0])
    assert int(sc.max()) >= 0.45 * (1 << 29) / 2, (case.label, int(sc.max()))


# ---- the extreme entry under an optimal path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", INT16_RULES)
def test_int16_families_use_their_extreme_entry(rule):
    """from the oracle's CIGARs on the batch the GPU test runs first: A/A lies under a ColM run wherever the set is about the
    maximum, A/C or N/G wherever it is about the minimum -- unless a mismatch of that size costs more than the two gaps around it
    (the lower end of the constant-gap profile rules, by the rule's own arithmetic; AffineGapLocal under a table without a positive
    entry, FP16 at gapExtend = - 7 999, which inserts the query whole): then the cell is read by the DP but is never chosen, and that
    is asserted instead"""
    checked = 0
    for c in env.cases(rule):
        if c.extreme is None:
            continue
        if rule == "N1":
            alphas, betas = env.n1_pairs(c.chunk)
            seen = set()
            for a, b in zip(alphas, betas):
                _, route = oracle.affine_gap_chunk(c.scores, c.gap_open, c.gap_extend, c.chunk, a, b)
                seen |= env.cells_under_path(a, b, [(r * c.chunk, o) for r, o in route])
        else:
            name = env.FIRST_SHAPES[rule] + (" level" if rule == "FP16" and c.gap_open >= 0 else "")
            if rule == "SS" and env.ss_is_key_family(c):
                alphas, betas = env.batch_total(c, rows=env.ss_key_rows(c.mode))
                seen = env.cells_of_batch(envo.expected(c, "sskeys", alphas, betas), alphas, betas)
            else:
                alphas, betas = env.batch_for(c, name)
                seen = env.cells_of_batch(envo.expected(c, name, alphas, betas), alphas, betas)
        if c.extreme in ("hi", "both"):
            assert env.HI_CELL in seen, c.label
        if c.extreme in ("lo", "both"):
            if env.min_reachable(c):
                assert any(lc in seen for lc in env.LO_CELLS), c.label
            else:
                # the DP reads the cell (an A of alpha and a C of beta in one pair) and no optimal path takes it
                assert any(env.A in a and env.C in b for a, b in zip(alphas, betas)), c.label
                assert not any(lc in seen for lc in env.LO_CELLS), c.label
        checked += 1
    assert checked >= 4
