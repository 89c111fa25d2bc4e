"""Tie-breaking, the part without a GPU: the census of tests/ties.py is the reference's walk (against tests/pyref.py on small pairs,
against the oracle on every batch), permuted orders of preference change exactly the pairs it predicts, and every batch
tests/test_ties_gpu.py runs meets -- on the reference's route alone -- the conditions that keep it from passing vacuously:
an I/D tie on at least half of the routes, every required class on at least 3 routes and 10 cells, a tied final state.  The control
keeps on record that the penalty sets of the route suites show none of this.  """
import collections

import numpy as np
import pytest

import common
import envelope
import oracle
import pyref
import ties
from ties import DIM, IMD, MDI, MID

BATCHES = [n for n in ties.PLAN if n != "diag"]


def _cases(name):
    for mode in ties.PLAN[name][0]:
        for sname in ties.plan_sets(name, mode):
            for ci in ties.checkers(name, mode):
                yield mode, sname, ci


def test_tables_and_admission():
    """the sets are what they are said to be, and every route they are run on admits them (tests/envelope.py's predicates)"""
    from gonomics_amd import align
    assert ties.HC2 == align.HumanChimpTwoScoreMatrix
    worst = min(v for row in ties.HC2[:4] for v in row[:4])
    for sname, (table, go, ge) in ties.AFFINE_SETS.items():
        two = 2 * (go + ge)
        lo = min(table[a][b] for a in range(4) for b in range(4) if a != b)
        hi = max(table[a][b] for a in range(4) for b in range(4) if a != b)
        assert (two == lo == hi) if sname == "tie15" else (two > hi), sname  # two gaps equal a mismatch, or beat every one
        for mode in ties.AFFINE_MODES:
            assert envelope.fp16(mode, table, go, ge) and envelope.gp16(mode, table, go, ge) and envelope.gp16(mode, table, go, ge, plain=True)
            assert envelope.p26(mode, table, go, ge) and envelope.k27(mode, table, go, ge, 3300, 3340)
            assert envelope.sn16(mode, table, go, ge) and envelope.spr_moving(mode, table, go, ge) and envelope.spr_w64(mode, table, go, ge)
    for sname, (table, g, _) in ties.CONST_SETS.items():
        lo = min(table[a][b] for a in range(4) for b in range(4) if a != b)
        assert (2 * g == lo) if sname == "tie15" else (2 * g > max(table[a][b] for a in range(4) for b in range(4) if a != b))
        for mode in (1, 4):
            assert envelope.cp16(mode, table, g, 0) and envelope.sn16(mode, table, g, 0) and envelope.k27(mode, table, g, 0, 3300, 3340)
            assert envelope.spr_moving(mode, table, g, 0) and envelope.spr_w64(mode, table, g, 0)
    assert 2 * (-600 - 150) < worst and 2 * -430 < worst  # the control: a mismatch is cheaper than two gaps


@pytest.fixture(scope="module")
def small_pairs():
    return common.random_pairs(911, 120, 1, 40, 1, 40)


@pytest.mark.parametrize("sname", list(ties.AFFINE_SETS) + ["control"])
def test_census_walk_vs_pyref_affine(small_pairs, sname):
    al, be = small_pairs
    table, go, ge = ties.params(0, sname)
    for mode, cs in ((0, 3), (0, 7), (2, 10000), (3, 10000)):
        got = ties.walk_batch(mode, table, go, ge, al, be, (cs,), (MID,))[(cs, MID)]
        for p, (a, b) in enumerate(zip(al, be)):
            exp = pyref.affine(a.tolist(), b.tolist(), table, go, ge, *((cs, cs) if mode == 0 else ()), free_end=(mode == 3))
            assert got[p][:2] == exp, (sname, mode, cs, p)
        common.assert_same(ties.as_result(got), oracle.align_batch(mode, table, go, ge, al, be, cs, cs), "%s mode %d cs %d" % (sname, mode, cs))


@pytest.mark.parametrize("sname", list(ties.CONST_SETS) + ["control"])
def test_census_walk_vs_pyref_const(small_pairs, sname):
    al, be = small_pairs
    table, g, _ = ties.params(1, sname)
    for mode, cs in ((1, 3), (1, 7), (4, 10000)):
        got = ties.walk_batch(mode, table, g, 0, al, be, (cs,), (MID,))[(cs, MID)]
        for p, (a, b) in enumerate(zip(al, be)):
            assert got[p][:2] == pyref.const(a.tolist(), b.tolist(), table, g, *((cs, cs) if mode == 1 else ())), (sname, mode, cs, p)
        common.assert_same(ties.as_result(got), oracle.align_batch(mode, table, g, 0, al, be, cs, cs), "%s mode %d cs %d" % (sname, mode, cs))


def test_census_against_a_reference_with_another_order(small_pairs):
    """pyref with its tmt replaced by another order of preference is the walk under that order; and census() counts, per pair, the
    classes on which the two orders part: none of them on a route <=> the CIGAR stays"""
    al, be = small_pairs
    table, go, ge = ties.AFFINE_SETS["hc70"]

    def tmt_mdi(a, b, c):
        return (a, 0) if a >= b and a >= c else ((c, 2) if c >= b else (b, 1))
    keep = pyref.tmt
    pyref.tmt = tmt_mdi
    try:
        swapped = [pyref.affine(a.tolist(), b.tolist(), table, go, ge, 3, 3) for a, b in zip(al, be)]
        swapped_c = [pyref.const(a.tolist(), b.tolist(), table, -70, 3, 3) for a, b in zip(al, be)]
    finally:
        pyref.tmt = keep
    got = ties.walk_batch(0, table, go, ge, al, be, (3,), (MID, MDI))
    got_c = ties.walk_batch(1, table, -70, 0, al, be, (3,), (MID, MDI))
    cen, cen_c = ties.census(0, table, go, ge, al, be, 3, 3), ties.census(1, table, -70, 0, al, be, 3, 3)
    differ = 0
    for p in range(len(al)):
        assert got[(3, MDI)][p][:2] == swapped[p] and got_c[(3, MDI)][p][:2] == swapped_c[p], p
        assert (got[(3, MDI)][p][1] != got[(3, MID)][p][1]) == any(t == "ID" for (_, t), v in cen[p].items() if v), p
        assert (got_c[(3, MDI)][p][1] != got_c[(3, MID)][p][1]) == (cen_c[p][("V", "ID")] > 0), p
        differ += got[(3, MDI)][p][1] != got[(3, MID)][p][1]
    assert differ >= len(al) // 4


def test_batch_shapes_and_composition():
    """the shapes the routes need (tests/asym.py's), nothing above 3 300 rows, 24 pairs or fewer in the long batches"""
    L = {n: ([len(a) for a in ties.batch(n)[0]], [len(b) for b in ties.batch(n)[1]]) for n in ties.PLAN}
    assert max(L["small"][0]) <= 160
    assert sum(n > 320 for n in L["long16"][0]) >= 6 and sum(n > 256 for n in L["tall12"][0]) >= 8 and all(n > m for n, m in zip(*L["tall12"]))
    assert min(L["coop"][1]) >= 1024 and any(n > 160 for n in L["coop"][0])
    assert len(L["long40"][0]) == 24 and min(L["long40"][0]) > 160
    assert 3 * sum(n > 1280 for n in L["w64"][0]) >= len(L["w64"][0])
    assert min(L["panels"][0]) > 1280 and max(L["panels"][0]) == 3300
    for k in (1, 2, 3):
        for name, side in (("fp%d" % k, 0), ("xp%d" % k, 1)):
            reads, wins = L[name][side], L[name][1 - side]
            assert min(reads) == 160 * (k - 1) + 1 and max(reads) == 160 * k and all(w <= r + 40 for r, w in zip(reads, wins))
    assert all(420 <= n <= 480 for n in L["diag"][0])
    for name, (ns, ms) in L.items():
        assert max(ns + ms) <= 3340 and len(ns) <= (24 if max(ns) > 480 else 36) and min(ns + ms) >= 1, name
    # a third of each batch per kind of sequence; in every kind, every other pair has its sides exchanged
    for name in ("small", "long40", "fp1"):
        al, be = ties.batch(name)
        top2 = [np.sort(np.bincount(np.concatenate([a, b]), minlength=5))[-2:].sum() / (len(a) + len(b)) for a, b in zip(al, be)]
        assert np.median(top2[1::3]) >= 0.85 and np.median(top2[0::3]) < 0.7, name  # two letters / four
        assert all(len(a) > 0 and a.max() <= 3 for a in al + be)


@pytest.mark.parametrize("name", BATCHES)
def test_batches_are_decisive(name):
    """the conditions of ties.decisive (which include: the census walk equals the oracle) for every batch, mode, set and checkerboard
    size the GPU module uses.  An exemption (ties.EXEMPT) stands only while the census shows the class out of reach of that batch
    under that set, and between them the sets of a batch require the whole table of classes"""
    asked, missed = collections.defaultdict(set), collections.defaultdict(set)
    for mode, sname, ci in _cases(name):
        assert ties.decisive(name, mode, sname, ci)
        asked[ties.kind_of(mode)].update(ties.required(name, mode, sname, ci))
        cnts = ties.counts(name, mode, sname, ci)
        missed[(ties.kind_of(mode), sname)].update(c for c in ties.full_table(name, mode, sname, ci) if not ties.reaches(cnts, c))
        if name[:2] in ("fp", "xp"):
            assert ties.staged(name, mode, sname, ci)
    for (kind, sname), miss in missed.items():
        stale = set(ties.EXEMPT.get((name, kind, sname), ())) - miss
        assert not stale, "%s %s %s reaches %s: require it" % (name, kind, sname, sorted(stale))
    for kind, got in asked.items():
        want = set(ties.family_table({"affine": 0, "local": 3, "const": 1}[kind]))
        if kind == "affine" and name in ties.SMALL_CHECKERS and 0 in ties.PLAN[name][0]:
            want |= set(ties.REQUIRED_Q1)
        assert want <= got, (name, kind, sorted(want - got))


def test_exemptions_name_batches_and_sets_that_exist():
    for (name, kind, sname), classes in ties.EXEMPT.items():
        mode = {"affine": 0, "local": 3, "const": 1}[kind]
        assert name in ties.PLAN and mode in ties.PLAN[name][0] and sname in ties.plan_sets(name, mode) and classes
        # what a set is run for is exempt nowhere: "MID" under the tie table, the M site's and V's two-way ties under the others
        core = {("M", "MID"), ("V", "MID")} if sname == "tie15" else {(site, t) for site in ("M", "V") for t in ("MI", "MD", "ID")}
        assert not core & set(classes), (name, kind, sname)


@pytest.mark.parametrize("name", list(ties.PLAN))
def test_permuted_orders_change_exactly_the_predicted_pairs(name):
    """(M, D, I) and two orders that demote M: the CIGAR of a pair changes if and only if its census holds a class the order decides
    otherwise.  Not vacuous: the wrong order (M, D, I) changes at least half of the pairs of every batch under every set in which
    two gaps beat a mismatch; under the tie table, where M is in nearly every such tie, (I, M, D) does"""
    for mode, sname, ci in _cases(name):
        cnts = ties.counts(name, mode, sname, ci)
        for order in (MDI, IMD, DIM):
            predicted = [any(v and ties.decided_otherwise(order, t) for (_, t), v in c.items()) for c in cnts]
            assert ties.changed(name, mode, sname, order, ci) == predicted, (name, mode, sname, ci, order)
        wrong = IMD if sname == "tie15" else MDI
        assert 2 * sum(ties.changed(name, mode, sname, wrong, ci)) >= len(cnts), (name, mode, sname, ci)


@pytest.mark.parametrize("name", BATCHES)
def test_control_the_old_sets_are_blind(name):
    """HumanChimpTwo (-600, -150) and ConstGap -430 on the same batches: no tie with I and D in it on at least 90 % of the routes, and
    the wrong order (M, D, I) changes at most those few -- what the route suites could not see"""
    for mode in ties.PLAN[name][0]:
        if mode in (2, 4):
            continue  # (the low-memory twin beyond every checkerboard edge is the same walk)
        assert ties.blind(name, mode) >= 0.9, (name, mode, ties.blind(name, mode))
        assert sum(ties.changed(name, mode, "control", MDI)) <= 0.1 * len(ties.batch(name)[0]), (name, mode)
        common.assert_same(ties.as_result(ties.runs(name, mode, "control")), ties.expected(name, mode, "control"), "control %s mode %d" % (name, mode))


def test_block_diag_batch():
    """three-block reads with an indel in the top block (no whole-read diagonal finishes the walk), whose route crosses the middle block
    on a plain diagonal while the indel could as well lie inside that block: an MI or MD tie at its M sites"""
    good = ties.diag_condition()
    assert len(good) >= 6
    assert np.all(np.diff(ties.expected("diag", 0, "tie15")[2]) <= 64)  # every CIGAR inside the runs the walk stages
    cnts = ties.counts("diag", 0, "tie15")
    assert all(c[("M", "MI")] + c[("M", "MD")] > 0 for c in cnts)
