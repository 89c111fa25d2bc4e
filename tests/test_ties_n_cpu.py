"""Tie-breaking in the chunk / group DPs (N1) and the seed-extension DPs (N2), the part without a GPU: the census of tests/ties_n.py
is the reference's walk (against literal cell-by-cell statements on small inputs, against the oracle on every batch, chunk and set
tests/test_ties_n_gpu.py runs), permuted orders of preference change exactly the pairs it predicts, every case meets -- on the
reference's route alone -- the conditions that keep it from passing vacuously, and the control keeps on record that the penalty
sets of tests/test_n1_gpu.py and tests/test_n2_gsw.py show none of this.  """
import collections

import numpy as np
import pytest

import common
import envelope
import oracle
import ties
import ties_n
from ties import DIM, IMD, MDI, MID

N1_CASES = [(name, chunk, sname) for (name, chunk), sets in ties_n.N1_PLAN.items() for sname in sets]
EXT_CASES = [(name, side, sname) for name, sets in ties_n.EXT_PLAN.items() for side in (0, 1) for sname in sets]


def _mismatches(table):
    return [table[a][b] for a in range(4) for b in range(4) if a != b]


def test_sets_and_admission():
    """the sets are what they are said to be, and every entry they are run on admits them: N1 (the int16 score matrix; the scaled
    set is the one that must fail it), K27 on the parameters the DP sees, SS for the score-only entries, and the right extension's
    packed maximum"""
    from gonomics_amd import align
    assert ties.HC2 == align.HumanChimpTwoScoreMatrix and ties_n.DEFAULT == align.DefaultScoreMatrix
    for (name, chunk), sets in ties_n.N1_PLAN.items():
        kinds = set()
        for sname in sets:
            table, go, ge = ties_n.n1_params(sname)
            if sname in ties_n.EQUAL_N1:  # a cell of `chunk` bases with k mismatches that equals two gaps of a chunk
                assert chunk in ties_n.EQUAL_AT[sname] and go == 0
                assert any(10 * chunk - 40 * k == 2 * ge * chunk for k in range(1, chunk + 1)), (sname, chunk)
                kinds.add("equal")
            else:  # two gaps of one cell beat every mismatch of the table
                assert 2 * (go + ge) > max(_mismatches(table)), sname
                kinds.add("beat")
            assert envelope.n1_s16(table, go, ge, chunk) == (not sname.endswith("x40")), (sname, chunk)
            seen_dp = [[v * chunk for v in row] for row in table]
            shapes = ties_n.C_SHAPES[name]() if name != "g_small" else [(b.shape[1] // chunk,) * 2 for b in ties_n.group_batch(chunk)[0]]
            big_n, big_m = max(n for n, _ in shapes), max(m for _, m in shapes)
            assert envelope.k27(2, seen_dp, go, ge * chunk, big_n, big_m) and envelope.p26(2, table, go, ge), (sname, chunk)
            assert envelope.ss(2, seen_dp, go, ge * chunk, big_n, big_m) == (not sname.endswith("x40")), (sname, chunk)
        assert kinds == {"beat", "equal"}, (name, chunk)
        assert any(s.endswith("x40") for s in sets) == ((name, chunk) in (("c_small", 5), ("g_small", 2)))
    for sname, (table, gap) in ties_n.EXT_SETS.items():
        assert (2 * gap == min(_mismatches(table)) == max(_mismatches(table))) if sname == "tie15" else (2 * gap > max(_mismatches(table)))
        worst = max(max(abs(v) for row in table for v in row), abs(gap))
        for name in list(ties_n.EXT_PLAN) + ["x_cross"]:
            for a, b in zip(*ties_n.ext_batch(name, 1)):
                assert len(a) <= 4095 and len(b) <= 4095 and (len(a) + len(b) + 2) * worst < (1 << 19), (name, sname)
        assert all(-32768 <= 4 * v + 3 <= 32767 for row in table for v in row)  # the int16 profile of the piped launch
    assert (1 << 19) // 356 == 1472
    worst = min(_mismatches(ties.HC2))
    assert 2 * (-600 - 150) < worst and 2 * -600 < worst and 2 * (-400 - 30) < min(_mismatches(ties_n.DEFAULT))  # the control


def _literal_scored(smat, go, ge, order):
    """or_scored_affine cell by cell in Python integers, its tripleMaxTrace under an order of preference"""
    n, m = smat.shape
    neg = -(1 << 50)

    def tmt(c):
        best = max(c)
        return best, next(k for k in order if c[k] == best)
    V = [[[neg] * (m + 1) for _ in range(n + 1)] for _ in range(3)]
    T = [[[0] * (m + 1) for _ in range(n + 1)] for _ in range(3)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 and j == 0:
                V[0][0][0], V[1][0][0], V[2][0][0] = 0, go, go
            elif i == 0:
                V[1][0][j], T[1][0][j] = ge + V[1][0][j - 1], 1
            elif j == 0:
                V[2][i][0], T[2][i][0] = ge + V[2][i - 1][0], 2
            else:
                s = int(smat[i - 1, j - 1])
                V[0][i][j], T[0][i][j] = tmt([s + V[k][i - 1][j - 1] for k in range(3)])
                V[1][i][j], T[1][i][j] = tmt([go + ge + V[0][i][j - 1], ge + V[1][i][j - 1], go + ge + V[2][i][j - 1]])
                V[2][i][j], T[2][i][j] = tmt([go + ge + V[0][i - 1][j], go + ge + V[1][i - 1][j], ge + V[2][i - 1][j]])
    score, k = tmt([V[x][n][m] for x in range(3)])
    ops, i, j = [], n, m
    while i > 0 or j > 0:
        ops.append(k)
        nk = T[k][i][j]
        i, j = i - (k != 1), j - (k != 2)
        k = nk
    return score, [(r, o) for r, o in reversed(ties_n._rle(ops))]


def test_census_walk_vs_literal_statements():
    """small inputs: the row-wise fill and the walk of ties_n against a cell-by-cell statement, under every order of preference
    (a reference with another tripleMaxTrace IS the walk under that order); the score matrices against the oracle's through the
    one-cell case; the extension walks against tests/test_n2_gsw.py's independent statement"""
    import test_n2_gsw
    rng = np.random.default_rng(912)
    for sname in ("hc3010", "tie15", "tie5"):
        table, go, ge = ties_n.n1_params(sname)
        for chunk in (1, 2, 3):
            for k in range(12):
                a, b = ties_n._chunk_pair(rng, k, int(rng.integers(1, 25)), int(rng.integers(1, 25)), chunk, 0.1, 0.1)
                smat = ties_n.chunk_matrix(table, chunk, a, b)
                got = ties_n.walk_scored(smat, go, ge, chunk, ties.ORDERS)
                for order in ties.ORDERS:
                    score, route = _literal_scored(smat, go, ge * chunk, order)
                    assert got[order][:2] == (score, [(r * chunk, o) for r, o in route]), (sname, chunk, k, order)
                assert got[MID][:2] == oracle.affine_gap_chunk(table, go, ge, chunk, a, b)
    # one cell of the group matrix is the oracle's score of a 1 x 1 call (M wins or loses against two gaps of 0)
    blocks, _ = ties_n.group_batch(2)
    for x, y in ((1, 3), (3, 1), (6, 7)):
        s = ties_n.group_matrix(ties_n.DEFAULT, 2, blocks[x][:, :6], blocks[y][:, :8])
        for i in range(3):
            for j in range(4):
                one = oracle.multiple_affine_gap(ties_n.DEFAULT, -100000, 0, 2, blocks[x][:, 2 * i:2 * i + 2], blocks[y][:, 2 * j:2 * j + 2])
                assert one == (int(s[i, j]), [(2, 0)]), (x, y, i, j)
    for sname in ties_n.EXT_SETS:
        table, gap = ties_n.ext_params(sname)
        for side in (0, 1):
            for k in range(16):
                a, b = ties_n._ext_pair(rng, k, int(rng.integers(1, 40)), int(rng.integers(1, 40)), side)
                V, code = ties_n.fill_ext(side, table, gap, a, b)
                assert ties_n.walk_ext(side, V, code, MID)[:4] == test_n2_gsw.py_gsw(side, a, b, table, gap) == oracle.gsw_extend(side, table, gap, a, b)


def test_batch_shapes_and_composition():
    """the shapes each kernel instantiation needs, from the batches themselves"""
    for name, chunks in ties_n.C_CHUNKS.items():
        for chunk in chunks:
            al, be = ties_n.chunk_batch(name, chunk)
            ns, ms = [len(a) // chunk for a in al], [len(b) // chunk for b in be]
            assert all(len(a) % chunk == 0 and len(b) % chunk == 0 and len(a) and len(b) for a, b in zip(al, be))
            assert list(zip(ns, ms)) == ties_n.C_SHAPES[name]()
            if name == "c_small":
                assert len(ns) == 24 and max(ns) == 160 and (1, 30) in zip(ns, ms) and (30, 1) in zip(ns, ms)  # one strip
            else:
                assert len(ns) == 10 and min(ns) > 160 and (321, 330) in zip(ns, ms) and (257, 300) in zip(ns, ms)
                assert sum(m >= 512 for m in ms) >= 2 and max(ns + ms) >= 256 and max(ns) <= 450 and max(ms) <= 600
            top2 = [np.sort(np.bincount(np.concatenate([a, b]), minlength=5))[-2:].sum() / (len(a) + len(b)) for a, b in zip(al, be)]
            assert np.median(top2[1::3]) >= 0.85 and np.median(top2[0::3]) < 0.7, (name, chunk)  # two letters / four
            assert all(a.max() <= 3 and b.max() <= 3 for a, b in zip(al, be))
    for chunk in ties_n.G_CHUNKS:
        blocks, pairs = ties_n.group_batch(chunk)
        assert len(blocks) == 8 and len(pairs) == 56 and sorted({b.shape[0] for b in blocks}) == [1, 2, 3, 4]
        assert all(40 <= b.shape[1] // chunk <= 200 and b.shape[1] % chunk == 0 for b in blocks) and max(b.shape[1] // chunk for b in blocks) > 160
        assert all((b[0] != ties_n.GAP).all() for b in blocks) and any((b == ties_n.GAP).any() for b in blocks)
        assert any(((b >= ties_n.LOWER) & (b < ties_n.GAP)).any() for b in blocks) and any((b < ties_n.LOWER).any() for b in blocks)
    for side in (0, 1):
        L = {n: ([len(a) for a in ties_n.ext_batch(n, side)[0]], [len(b) for b in ties_n.ext_batch(n, side)[1]]) for n in ties_n.EXT_PLAN}
        assert len(L["x_small"][0]) == 30 and max(L["x_small"][0]) == 160 and max(L["x_small"][1]) <= 150
        assert len(L["x_multi"][0]) == 12 and min(L["x_multi"][0]) == 161 and {320, 321} <= set(L["x_multi"][0]) and max(L["x_multi"][0]) <= 700
        assert max(L["x_multi"][1]) < 512 and min(L["x_multi"][1]) >= 100
        assert len(L["x_piped"][0]) == 8 and min(L["x_piped"][0]) >= 170 and max(L["x_piped"][0]) <= 600 and min(L["x_piped"][1]) >= 512 and max(L["x_piped"][1]) <= 800
        assert all(n + m + 2 <= 1472 for n, m in zip(*L["x_piped"]))


@pytest.mark.parametrize("name,chunk,sname", N1_CASES)
def test_n1_cases_are_decisive(name, chunk, sname):
    """ties_n.decisive_n1 (which includes: the census walk equals the oracle) for every case the GPU module runs, and no stale
    exemption: an exempt class must be out of the batch's reach under that set"""
    assert ties_n.decisive_n1(name, chunk, sname)
    cnts = ties_n.n1_counts(name, chunk, sname)
    stale = [c for c in ties_n.EXEMPT_N1.get((name, chunk, sname), ()) if ties.reaches(cnts, c)]
    assert not stale, "%s chunk %d %s reaches %s: require it" % (name, chunk, sname, stale)


@pytest.mark.parametrize("name,side,sname", EXT_CASES)
def test_ext_cases_are_decisive(name, side, sname):
    assert ties_n.decisive_ext(name, side, sname)
    cnts = ties_n.ext_counts(name, side, sname)
    stale = [c for c in ties_n.EXEMPT_EXT.get((name, side, sname), ()) if ties.reaches(cnts, c)]
    assert not stale, "%s side %d %s reaches %s: require it" % (name, side, sname, stale)


def test_exemptions_and_sets_not_run():
    """the exemptions name cases that exist and never the class a set is run for; no batch is exempt from a class under every
    set it runs; the sets listed as not run do fail the conditions where they are not run"""
    asked = collections.defaultdict(set)
    for name, chunk, sname in N1_CASES:
        asked[name].update(ties_n.required_n1(name, chunk, sname))
    for name, side, sname in EXT_CASES:
        asked[(name, side)].update(ties_n.required_ext(name, side, sname))
    for key, got in asked.items():
        want = set(ties_n.REQUIRED_N1 if isinstance(key, str) else ties_n.REQUIRED_EXT)
        assert want <= got, (key, sorted(want - got))
    for (name, chunk, sname), classes in ties_n.EXEMPT_N1.items():
        assert (name, chunk, sname) in N1_CASES and classes
        # what a set is run for is exempt nowhere: "MID" at the M site where two gaps equal a cell score, I against D there elsewhere
        core = {("M", "MID")} if sname in ties_n.EQUAL_N1 else {("M", "ID")}
        if (name, chunk, sname) == ("c_small", 3, "tie15"):
            core = set()  # (the equal cell of chunk 3 has all three bases mismatched: 5 cells of the short batch; c_long has it)
        assert not core & set(classes), (name, chunk, sname)
    for (name, side, sname), classes in ties_n.EXEMPT_EXT.items():
        assert (name, side, sname) in EXT_CASES and classes
        core = {("V", "MID")} if sname == "tie15" else {("V", "MI"), ("V", "MD"), ("V", "ID")}
        assert not core & set(classes), (name, side, sname)
    for (name, chunk), sname in ties_n.NOT_RUN:
        assert sname not in ties_n.N1_PLAN[(name, chunk)]
        with pytest.raises(AssertionError):
            ties_n.decisive_n1(name, chunk, sname)


@pytest.mark.parametrize("family", ["n1", "ext"])
def test_permuted_orders_change_exactly_the_predicted_pairs(family):
    """(M, D, I) and two orders that demote M: the result of a pair changes if and only if its census holds a class the order
    decides otherwise (for the extensions the result includes the end of the walk).  That the wrong order changes at least half of
    the pairs of every case is part of decisive_*"""
    for name, key, sname in (N1_CASES if family == "n1" else EXT_CASES):
        cnts = ties_n.n1_counts(name, key, sname) if family == "n1" else ties_n.ext_counts(name, key, sname)
        for order in (MDI, IMD, DIM):
            predicted = [any(v and ties.decided_otherwise(order, t) for (_, t), v in c.items()) for c in cnts]
            changed = ties_n.n1_changed(name, key, sname, order) if family == "n1" else ties_n.ext_changed(name, key, sname, order)
            assert changed == predicted, (name, key, sname, order)


def test_control_the_present_sets_are_blind():
    """HumanChimpTwo (-600, -150) on the chunk batches, the default table with (-400, -30) on the groups, gap -600 on the
    extensions: the wrong order (M, D, I) changes at most a tenth of the pairs of any batch -- what tests/test_n1_gpu.py and
    tests/test_n2_gsw.py could not see.  The census walk is the oracle there too"""
    for name, ctl in ties_n.CONTROL_OF.items():
        for chunk in ties_n.C_CHUNKS.get(name, ties_n.G_CHUNKS):
            for sname in ctl:
                changed = ties_n.n1_changed(name, chunk, sname, MDI)
                assert sum(changed) <= 0.1 * len(changed), (name, chunk, sname, sum(changed))
                ties_n._same_n1(ties_n.n1_runs(name, chunk, sname)[MID], ties_n.n1_expected(name, chunk, sname), "control %s %d %s" % (name, chunk, sname))
    for name in ties_n.EXT_PLAN:
        for side in (0, 1):
            changed = ties_n.ext_changed(name, side, "c600", MDI)
            assert sum(changed) <= 0.1 * len(changed), (name, side, sum(changed))
            assert [r[:4] for r in ties_n.ext_runs(name, side, "c600")[0][MID]] == ties_n.ext_expected(name, side, "c600")


def test_constructed_right_extension_pairs():
    """the maximum in exactly two cells of different rows, in the same strip and in neighbouring strips; the oracle ends at the first"""
    assert ties_n.cross_condition() == ((100, 100), (330, 330), (300, 300))
