"""The score-only chunk / multiple-alignment entries on the GPU (gnx_affine_gap_chunk_score_batch, gnx_multiple_affine_gap_score_batch;
the sweep of n1_sweep.hip.h, fast_path 9) against the oracle, their fallbacks and errors against the align twins, and the score-first
progressive driver (AllSeqAffine, AllSeqAffineChunk, cmds.faChunkAlign) against golden G8 and the oracle.  Lengths are in chunk cells."""
import os

import numpy as np
import pytest

import common
import n1_helpers
import oracle
from gonomics_amd import align, cmds, dna, fasta

pytestmark = pytest.mark.gpu
MX = common.matrices()
D = os.path.join(common.DATA, "align")


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    """the switches that choose between the sweep and the twin's route are the tests' own"""
    for k in ("GNX_SCORE_SWEEP", "GNX_WIDE", "GNX_N1_SCORE_FIRST"):
        monkeypatch.delenv(k, raising=False)


def _route(lib):
    return lib.get_timing()["fast_path"]


def _seq(rng, cells, chunk, alphabet=5):
    return rng.integers(0, alphabet, size=cells * chunk).astype(np.uint8)


def _pair(rng, n, m, chunk, alphabet=5):
    """two sequences of n and m chunk cells, related half of the time (so that the diagonal matters)"""
    a = _seq(rng, n, chunk, alphabet)
    if rng.random() < 0.5:
        b = common.mutate(rng, a, sub=0.1, indel=0.05, geo=0.4, alphabet=alphabet)
        b = np.concatenate([b, _seq(rng, m, chunk, alphabet)])[:m * chunk]
    else:
        b = _seq(rng, m, chunk, alphabet)
    return a, b


def _check_pairs(lib, scores, go, ge, chunk, alphas, betas, what, route=9):
    p = lib.make_params(lib.GNX_AFFINE_GAP_HIGHMEM, scores, go, ge)
    got = lib.affine_gap_chunk_score_batch(p, chunk, alphas, betas)
    assert _route(lib) == route, (what, _route(lib))
    for k, (a, b) in enumerate(zip(alphas, betas)):
        exp = oracle.affine_gap_chunk(scores, go, ge, chunk, a, b)[0]
        assert int(got[k]) == exp, (what, k, len(a) // chunk, len(b) // chunk, int(got[k]), exp)


def test_fuzz_pairs(gpu_lib):
    """single sequences: chunk 1, 2, 3 (the column-walking matrix kernel) and 5 (the generic one); batches of 1, 4 and 5 pairs (a full
    quad and a partial one) with mixed lengths inside a quad, either side the longer one"""
    rng = np.random.default_rng(31)
    for chunk in (1, 2, 3, 5):
        for batch in (1, 4, 5):
            alphas, betas = [], []
            for _ in range(batch):
                a, b = _pair(rng, int(rng.integers(1, 400)), int(rng.integers(1, 400)), chunk)
                alphas.append(a); betas.append(b)
            _check_pairs(gpu_lib, MX["HumanChimpTwo"], -600, -150, chunk, alphas, betas, ("pairs", chunk, batch))


def _group(rng, nseq, cells, chunk):
    blk = rng.integers(0, 10, size=(nseq, cells * chunk)).astype(np.uint8)  # upper + lower case
    blk[rng.random(blk.shape) < 0.1] = dna.Gap
    blk[0, blk[0] == dna.Gap] = 1  # one member without gaps: no column pair is gap-only
    return blk


def test_fuzz_groups(gpu_lib):
    """groups of 1 .. 4 members with lower case and gaps: chunk 1, 2, 3 (column profiles) and 5 (the generic matrix kernel)"""
    rng = np.random.default_rng(32)
    for chunk in (1, 2, 3, 5):
        groups = [_group(rng, int(rng.integers(1, 5)), int(rng.integers(1, 260)), chunk) for _ in range(5)]
        groups.append(_group(rng, 1, 7, chunk))
        every = [(x, y) for x in range(len(groups)) for y in range(len(groups)) if x != y]
        for batch in (1, 4, 5):
            pairs = [every[int(k)] for k in rng.choice(len(every), size=batch, replace=False)]
            p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.DefaultScoreMatrix, -400, -30)
            got = gpu_lib.multiple_affine_gap_score_batch(p, chunk, groups, pairs)
            assert _route(gpu_lib) == 9, (chunk, batch)
            for k, (x, y) in enumerate(pairs):
                exp = oracle.multiple_affine_gap(MX["Default"], -400, -30, chunk, groups[x], groups[y])[0]
                assert int(got[k]) == exp, (chunk, batch, x, y, groups[x].shape, groups[y].shape)
        assert align.multipleAffineGapScoreBatch([[fasta.Fasta("a", groups[5][0])], [fasta.Fasta("b", groups[0][0])]], [(0, 1)], align.DefaultScoreMatrix, -400, -30, chunk) == \
            [oracle.multiple_affine_gap(MX["Default"], -400, -30, chunk, groups[5][:1], groups[0][:1])[0]]


SHORT = (1, 9, 10, 11, 159, 160, 161, 320, 321, 481)  # lane, block and level boundaries: one, two, three and four levels
LONG = (15, 16, 17, 31, 32, 33, 200)                  # the 16-column chunks and the hand-over ring of 32


def _edge_pairs(chunk):
    rng = np.random.default_rng(33)
    alphas, betas = [], []
    for s in SHORT:
        for l in LONG:
            longer = l if l >= s else s + l  # (the longer side keeps the column count's remainder classes)
            a, b = _pair(rng, s, longer, chunk, alphabet=4)
            alphas.append(a); betas.append(b)   # beta longer
            a, b = _pair(rng, longer, s, chunk, alphabet=4)
            alphas.append(a); betas.append(b)   # alpha longer: the sides swap
    return alphas, betas


@pytest.fixture(scope="module")
def edge_pairs():
    al, be = _edge_pairs(1)
    return al, be, [oracle.affine_gap_chunk(MX["HumanChimpTwo"], -600, -150, 1, a, b)[0] for a, b in zip(al, be)]


@pytest.mark.parametrize("launch", ["piped", "level_by_level"])
def test_edges_of_the_geometry(gpu_lib, edge_pairs, launch, monkeypatch):
    """every (shorter, longer) combination in one batch (quads of mixed lengths and levels, whole blocks of padding), odd row counts
    (a lane's entries off a multiple of four rows), both sides as the longer one; the levels in one launch and level by level"""
    if launch == "level_by_level":
        monkeypatch.setenv("GNX_NO_PIPE", "1")
    al, be, exp = edge_pairs
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, MX["HumanChimpTwo"], -600, -150)
    got = gpu_lib.affine_gap_chunk_score_batch(p, 1, al, be)
    assert _route(gpu_lib) == 9
    bad = [(k, len(al[k]), len(be[k]), int(got[k]), exp[k]) for k in range(len(al)) if int(got[k]) != exp[k]]
    assert not bad, bad[:10]
    # each shape alone as well (a quad with three empty slots), for the level boundaries
    for k in (0, 2 * 7 * 4 + 1, 2 * 7 * 6 + 6, 2 * 7 * 8, 2 * 7 * 9 + 13):
        got1 = gpu_lib.affine_gap_chunk_score_batch(p, 1, [al[k]], [be[k]])
        assert int(got1[0]) == exp[k] and _route(gpu_lib) == 9, (k, len(al[k]), len(be[k]))


def test_edges_with_chunk_three(gpu_lib):
    al, be = _edge_pairs(3)
    _check_pairs(gpu_lib, MX["Default"], -400, -30, 3, al[::3], be[::3], "edges, chunk 3")


def test_ties_and_penalties(gpu_lib):
    rng = np.random.default_rng(34)
    alphas, betas = [], []
    for n, m in ((40, 40), (7, 300), (170, 165), (330, 45), (1, 1)):
        a, b = _pair(rng, n, m, 2, alphabet=2)  # two-letter sequences: many equal scores
        alphas.append(a); betas.append(b)
    for go, ge in ((0, 0), (-400, -30), (-7, -3), (0, -30), (-400, 0)):
        _check_pairs(gpu_lib, MX["Default"], go, ge, 2, alphas, betas, ("ties", go, ge))
    flat = [[1] * 5 for _ in range(5)]
    _check_pairs(gpu_lib, flat, 0, 0, 2, alphas, betas, "one score everywhere")


def test_fallbacks_equal_the_twin_and_report_its_route(gpu_lib, monkeypatch):
    rng = np.random.default_rng(35)
    alphas, betas = [], []
    for n, m in ((30, 50), (170, 20), (5, 5), (64, 200)):
        a, b = _pair(rng, n, m, 5)
        alphas.append(a); betas.append(b)

    def both(scores, go, ge, al, be, env=None):
        if env:
            monkeypatch.setenv(*env)
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, scores, go, ge)
        sc, _, _ = gpu_lib.affine_gap_chunk_batch(p, 5, al, be)
        twin_route = _route(gpu_lib)
        got = gpu_lib.affine_gap_chunk_score_batch(p, 5, al, be)
        route = _route(gpu_lib)
        if env:
            monkeypatch.delenv(env[0])
        assert [int(x) for x in got] == [int(x) for x in sc], (go, env)
        assert [int(x) for x in got] == [oracle.affine_gap_chunk(scores, go, ge, 5, a, b)[0] for a, b in zip(al, be)], (go, env)
        assert route != 9 and route == twin_route, (go, env, route, twin_route)

    both(MX["HumanChimpTwo"], 50, -150, alphas, betas)                                            # gapOpen > 0
    both(MX["HumanChimpTwo"], -600, -150, alphas + [alphas[0][:0]], betas + [betas[0]])            # an empty side
    both([[v * 40 for v in row] for row in align.HumanChimpTwoScoreMatrix], -600, -150, alphas, betas)  # s - 2e beyond +-16 000
    both(MX["HumanChimpTwo"], -600, -150, alphas, betas, env=("GNX_SCORE_SWEEP", "0"))
    both(MX["HumanChimpTwo"], -600, -150, alphas, betas, env=("GNX_WIDE", "2"))
    # ... and the same batch is the sweep's once nothing stands in the way
    _check_pairs(gpu_lib, MX["HumanChimpTwo"], -600, -150, 5, alphas, betas, "after the fallbacks")
    # groups: gapOpen > 0
    groups = [_group(rng, 2, 40, 1), _group(rng, 3, 55, 1)]
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.DefaultScoreMatrix, 10, -30)
    sc, _, _ = gpu_lib.multiple_affine_gap_batch(p, 1, groups, [(0, 1), (1, 0)])
    twin_route = _route(gpu_lib)
    got = gpu_lib.multiple_affine_gap_score_batch(p, 1, groups, [(0, 1), (1, 0)])
    assert [int(x) for x in got] == [int(x) for x in sc] and _route(gpu_lib) == twin_route != 9


def test_errors_equal_the_twins_code(gpu_lib):
    def code(fn, *args):
        with pytest.raises(gpu_lib.GnxError) as ei:
            fn(*args)
        return ei.value.code

    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.DefaultScoreMatrix, -400, -30)
    a, b = dna.StringToBases("ACGTACGTAC"), dna.StringToBases("ACGTTCGTAC")
    bad = a.copy(); bad[3] = 7
    for al, be in (([bad], [b]), ([a, a], [b, bad])):  # a base >= 5, on either side
        assert code(gpu_lib.affine_gap_chunk_score_batch, p, 2, al, be) == code(gpu_lib.affine_gap_chunk_batch, p, 2, al, be) == gpu_lib.GNX_EBASE
    gap = np.full((1, 6), dna.Gap, np.uint8)
    ok = np.stack([a[:6]])
    for chunk in (1, 3):  # column profiles (chunk <= 4) ...
        assert code(gpu_lib.multiple_affine_gap_score_batch, p, chunk, [gap, gap, ok], [(2, 2), (0, 1)]) == \
            code(gpu_lib.multiple_affine_gap_batch, p, chunk, [gap, gap, ok], [(2, 2), (0, 1)]) == gpu_lib.GNX_EDIVZERO
    gap5, ok5 = np.full((1, 10), dna.Gap, np.uint8), np.stack([a])  # ... and the generic matrix kernel
    assert code(gpu_lib.multiple_affine_gap_score_batch, p, 5, [gap5, ok5], [(1, 1), (0, 0)]) == code(gpu_lib.multiple_affine_gap_batch, p, 5, [gap5, ok5], [(1, 1), (0, 0)]) == gpu_lib.GNX_EDIVZERO
    assert code(gpu_lib.affine_gap_chunk_score_batch, p, 3, [a], [b]) == code(gpu_lib.affine_gap_chunk_batch, p, 3, [a], [b]) == gpu_lib.GNX_EINVAL
    assert code(gpu_lib.multiple_affine_gap_score_batch, p, 4, [ok, ok], [(0, 1)]) == code(gpu_lib.multiple_affine_gap_batch, p, 4, [ok, ok], [(0, 1)]) == gpu_lib.GNX_EINVAL
    with pytest.raises(IndexError):  # what align.py makes of GNX_EBASE (Go: index out of range)
        align.AffineGapChunkScore(bad, b, align.DefaultScoreMatrix, -400, -30, 2)
    assert align.AffineGapChunkScore(a, b, align.DefaultScoreMatrix, -400, -30, 2) == oracle.affine_gap_chunk(MX["Default"], -400, -30, 2, a, b)[0]


def _fa_bytes(records, path):
    fasta.Write(str(path), records)
    return open(str(path), "rb").read()


def test_command_outputs_with_and_without_score_first(gpu_lib, tmp_path, monkeypatch):
    """golden G8 (align/multiAlign_test.go:20-38) through AllSeqAffine and AllSeqAffineChunk, cmds.faChunkAlign against the oracle's
    progressive alignment: GNX_N1_SCORE_FIRST unset, 0 (every pair aligned every round) and 1 (score first) give the same bytes"""
    outs = {}
    for setting in (None, "0", "1"):
        if setting is None:
            monkeypatch.delenv("GNX_N1_SCORE_FIRST", raising=False)
        else:
            monkeypatch.setenv("GNX_N1_SCORE_FIRST", setting)
        res = []
        for inp, exp in (("multiAlignTest.in.fa", "multiAlignTest.expected.fa"), ("multiAlignTest.in2.fa", "multiAlignTest.expected2.fa")):
            records = fasta.Read(os.path.join(D, inp))
            expected = fasta.Read(os.path.join(D, exp))
            got1 = align.AllSeqAffine(records, align.DefaultScoreMatrix, -400, -30)
            got2 = align.AllSeqAffineChunk(records, align.DefaultScoreMatrix, -400, -30, 2)
            assert fasta.AllAreEqualIgnoreOrder(got1, expected) and fasta.AllAreEqualIgnoreOrder(got2, expected), (setting, inp)
            res += [_fa_bytes(got1, tmp_path / "a.fa"), _fa_bytes(got2, tmp_path / "b.fa")]
        out = tmp_path / "cmd.fa"
        got = cmds.faChunkAlign(os.path.join(D, "multiAlignTest.in.fa"), 2, -300, -40, str(out))
        exp = n1_helpers.all_seq_affine_oracle(fasta.Read(os.path.join(D, "multiAlignTest.in.fa")), MX["HumanChimpTwo"], -300, -40, 2)
        assert open(str(out), "rb").read() == _fa_bytes(exp, tmp_path / "exp.fa") == _fa_bytes(got, tmp_path / "got.fa"), setting
        res.append(open(str(out), "rb").read())
        outs[setting] = res
    assert outs[None] == outs["0"] == outs["1"]


def test_score_first_random_records_vs_oracle(gpu_lib, tmp_path, monkeypatch):
    monkeypatch.setenv("GNX_N1_SCORE_FIRST", "1")
    rng = np.random.default_rng(36)
    base = rng.integers(0, 4, size=90).astype(np.uint8)
    records = []
    for k in range(6):
        s = common.mutate(rng, base, sub=0.15, indel=0.05, geo=0.4, alphabet=4)
        s = np.concatenate([s, rng.integers(0, 4, size=90).astype(np.uint8)])[:90]
        records.append(fasta.Fasta("r%d" % k, s))
    got = align.AllSeqAffineChunk(records, align.HumanChimpTwoScoreMatrix, -300, -40, 3)
    exp = n1_helpers.all_seq_affine_oracle(records, MX["HumanChimpTwo"], -300, -40, 3)
    assert _fa_bytes(got, tmp_path / "got.fa") == _fa_bytes(exp, tmp_path / "exp.fa")
