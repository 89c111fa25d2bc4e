"""N1 on the GPU: AffineGapChunk, multipleAffineGap(Chunk) batches and AllSeqAffine(Chunk) through the C ABI,
against golden G8 and the oracle."""
import os

import numpy as np
import pytest

import common
import n1_helpers
import oracle
from gonomics_amd import align, dna, fasta

pytestmark = pytest.mark.gpu
T = common.tables()
MX = common.matrices()
D = os.path.join(common.DATA, "align")


@pytest.fixture(autouse=True, params=["lat", "general"])
def geometry(request, monkeypatch):
    """every test twice: small batches take the latency geometry by the library's routing (lat_fill_kernel<.., SCORED>: the score matrix through
    a register ring), GNX_LAT=0 keeps them on fill_affine_kernel<.., SCORED> -- unless a switch from outside has chosen already"""
    if "GNX_LAT" not in os.environ and request.param == "general":
        monkeypatch.setenv("GNX_LAT", "0")
    return request.param


def _route(r):
    return [(c.RunLength, c.Op) for c in r]


def test_affine_gap_chunk(gpu_lib):  # align/affineGap_test.go:83-93
    t = T["affineAlignChunkTests"]
    for c in t["cases"]:
        a, b = dna.StringToBases(c["seqOne"]), dna.StringToBases(c["seqTwo"])
        _, cigar = align.AffineGapChunk(a, b, align.DefaultScoreMatrix, -400, -30, 3)
        assert align.View(a, b, cigar) == c["aln"]


def test_affine_gap_multi(gpu_lib):  # align/affineGap_test.go:95-108
    t = T["affineAlignTests"]
    for c in t["cases"]:
        one = [fasta.Fasta("one", dna.StringToBases(c["seqOne"]))]
        two = [fasta.Fasta("two", dna.StringToBases(c["seqTwo"]))]
        (_, cigar), = align.multipleAffineGapBatch([one, two], [(0, 1)], align.DefaultScoreMatrix, -400, -30)
        answer = align.mergeMultipleAlignments(one, two, cigar)
        assert dna.BasesToString(answer[0].Seq) + "\n" + dna.BasesToString(answer[1].Seq) + "\n" == c["aln"]


def test_multi_align_gap(gpu_lib):  # align/multiAlign_test.go:20-38
    for inp, exp in (("multiAlignTest.in.fa", "multiAlignTest.expected.fa"), ("multiAlignTest.in2.fa", "multiAlignTest.expected2.fa")):
        records = fasta.Read(os.path.join(D, inp))
        expected = fasta.Read(os.path.join(D, exp))
        assert fasta.AllAreEqualIgnoreOrder(align.AllSeqAffine(records, align.DefaultScoreMatrix, -400, -30), expected)
        assert fasta.AllAreEqualIgnoreOrder(align.AllSeqAffineChunk(records, align.DefaultScoreMatrix, -400, -30, 2), expected)


def test_chunk_fuzz_vs_oracle(gpu_lib):
    rng = np.random.default_rng(8)
    for chunk in (1, 2, 3, 5):
        alphas, betas = [], []
        for _ in range(60):
            na, nb = int(rng.integers(0, 70)), int(rng.integers(0, 90))
            a = rng.integers(0, 5, size=na * chunk).astype(np.uint8)
            b = common.mutate(rng, a, sub=0.1, indel=0.05, geo=0.4, alphabet=5) if rng.random() < 0.6 and na else rng.integers(0, 5, size=nb * chunk).astype(np.uint8)
            b = b[:(len(b) // chunk) * chunk]
            alphas.append(a); betas.append(b)
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.HumanChimpTwoScoreMatrix, -600, -150)
        sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
        for k, (a, b) in enumerate(zip(alphas, betas)):
            exp = oracle.affine_gap_chunk(MX["HumanChimpTwo"], -600, -150, chunk, a, b)
            got = (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])
            assert got == exp, (chunk, k)
    # scores too large for the int16 score matrix (4 * chunk * max|score| > 32767): the int32 matrix, same answers
    big = [[v * 40 for v in row] for row in align.HumanChimpTwoScoreMatrix]
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, big, -24000, -6000)
    sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, 5, alphas, betas)
    for k, (a, b) in enumerate(zip(alphas, betas)):
        exp = oracle.affine_gap_chunk(big, -24000, -6000, 5, a, b)
        got = (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])
        assert got == exp, ("int32 matrix", k)


def test_chunk_batch_in_sub_batches(gpu_lib, monkeypatch):
    """Big inputs cross PCIe in sub-batches while the DP of the sub-batch before runs (run_host_scored; by itself only from 16 384
    pairs and 8 MB on, GNX_SCORED_SUB forces it): same results as the one-batch flow, a sample against the oracle; ragged lengths,
    empty pairs, a bad base in the last sub-batch -> GNX_EBASE."""
    rng = np.random.default_rng(21)
    chunk, pairs = 3, 700
    alphas, betas = [], []
    for k in range(pairs):
        nb = int(rng.integers(300, 900)) if k % 97 else 0
        b = rng.integers(0, 4, size=nb * chunk).astype(np.uint8)
        na = int(rng.integers(0, 200)) if nb else int(rng.integers(0, 3))
        s0 = int(rng.integers(0, max(nb - na, 1))) * chunk
        a = common.mutate(rng, b[s0:s0 + na * chunk], sub=0.05, indel=0.02, geo=0.4, alphabet=4) if na and nb else rng.integers(0, 4, size=na * chunk).astype(np.uint8)
        a = a[:(len(a) // chunk) * chunk]
        alphas.append(a); betas.append(b)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.HumanChimpTwoScoreMatrix, -600, -150)
    monkeypatch.setenv("GNX_SCORED_SUB", "1")
    sc1, ops1, off1 = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
    for sub in ("4", "7"):
        monkeypatch.setenv("GNX_SCORED_SUB", sub)
        sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
        assert np.array_equal(sc, sc1) and np.array_equal(off, off1), sub
        assert np.array_equal(ops["run_length"][:off[-1]], ops1["run_length"][:off1[-1]]) and np.array_equal(ops["op"][:off[-1]], ops1["op"][:off1[-1]]), sub
    for k in list(range(0, pairs, 131)) + [96, 97, 98, pairs - 1]:
        exp = oracle.affine_gap_chunk(MX["HumanChimpTwo"], -600, -150, chunk, alphas[k], betas[k])
        got = (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])
        assert got == exp, k
    betas[pairs - 2] = betas[pairs - 2].copy(); betas[pairs - 2][5] = 7
    with pytest.raises((gpu_lib.GnxError, IndexError)):
        gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
    monkeypatch.delenv("GNX_SCORED_SUB")


def test_groups_fuzz_vs_oracle(gpu_lib):
    rng = np.random.default_rng(9)
    for chunk in (1, 2):
        groups = []
        for _ in range(10):
            nseq, ln = int(rng.integers(1, 5)), int(rng.integers(1, 200)) * chunk
            blk = rng.integers(0, 10, size=(nseq, ln)).astype(np.uint8)  # upper + lower case
            blk[rng.random(blk.shape) < 0.1] = dna.Gap
            blk[0, blk[0] == dna.Gap] = 1  # keep one sequence gap-free so no column pair is gap-only
            groups.append(blk)
        pairs = [(x, y) for x in range(len(groups)) for y in range(len(groups)) if x != y]
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.DefaultScoreMatrix, -400, -30)
        sc, ops, off = gpu_lib.multiple_affine_gap_batch(p, chunk, groups, pairs)
        for k, (x, y) in enumerate(pairs):
            exp = oracle.multiple_affine_gap(MX["Default"], -400, -30, chunk, groups[x], groups[y])
            got = (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])
            assert got == exp, (chunk, x, y)


def test_n1_errors(gpu_lib):
    with pytest.raises(gpu_lib.GnxError):  # length not a multiple of the chunk size -> log.Fatalf in Go
        align.AffineGapChunk(dna.StringToBases("ACGT"), dna.StringToBases("ACG"), align.DefaultScoreMatrix, -400, -30, 3)
    gap = [fasta.Fasta("g", np.full(4, dna.Gap, np.uint8))]
    with pytest.raises(gpu_lib.GnxError):  # integer divide by zero in scoreColumnMatch
        align.multipleAffineGapBatch([gap, gap], [(0, 1)], align.DefaultScoreMatrix, -400, -30)
    with pytest.raises(IndexError):  # lower-case bases index past the matrix in the pairwise chunk variant
        align.AffineGapChunk(dna.StringToBases("ACgT"), dna.StringToBases("ACGT"), align.DefaultScoreMatrix, -400, -30, 2)


def test_fa_chunk_align_command(gpu_lib, tmp_path):  # cmd/faChunkAlign/faChunkAlign.go:18-29: read multi-fasta, AllSeqAffineChunk(HumanChimpTwo), write
    from gonomics_amd import cmds
    out = str(tmp_path / "aligned.fa")
    records = fasta.Read(os.path.join(D, "multiAlignTest.in.fa"))
    got = cmds.faChunkAlign(os.path.join(D, "multiAlignTest.in.fa"), 2, -300, -40, out)
    exp = align.AllSeqAffineChunk(records, align.HumanChimpTwoScoreMatrix, -300, -40, 2)
    assert fasta.AllAreEqualIgnoreOrder(got, exp) and fasta.AllAreEqualIgnoreOrder(fasta.Read(out), exp)
    assert len({len(r.Seq) for r in got}) == 1  # an alignment: equal lengths


def _n1_got(sc, ops, off, k):
    return (int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])])


def _all_empty_batches(chunk, cells):
    """batches in which EVERY pair has an empty side (the scored int64 route then has no strip to fill: the traceback's closed forms alone):
    one pair with an empty alpha, the same pair with the sides swapped, three pairs with one empty side each"""
    rng = np.random.default_rng(4242)
    empty = np.zeros(0, np.uint8)
    long_one, other = rng.integers(0, 5, size=cells * chunk).astype(np.uint8), rng.integers(0, 5, size=(cells // 2 + 1) * chunk).astype(np.uint8)
    return [([empty], [long_one]), ([long_one], [empty]), ([empty, long_one, empty], [long_one, empty, other])]


def test_n1_beyond_int32(gpu_lib, geometry):
    """round 6: the chunk / multiple-alignment variants have no GNX_ERANGE any more -- the reference is int64 there too
    (align/affineGap_highMem.go:227-353).  A call with a pair whose keys 4 * score leave the static int32 range runs on the int64 kernel with explicit
    score matrices (lat_wide_kernel<.., SCORED>): scores x 4 000 (keys to 6e9) on ragged pairs, one pair of 2e6 chunk cells, groups with scaled scores --
    all against the oracle."""
    if geometry == "general":
        pytest.skip("the int64 kernel has one geometry")
    rng = np.random.default_rng(88)
    x1000 = [[v * 4000 for v in row] for row in align.HumanChimpTwoScoreMatrix]  # (x 4 000: the name is from the first draft)
    chunk = 3
    alphas, betas = [], []
    for k in range(24):
        na, nb = int(rng.integers(0, 300)), int(rng.integers(1, 400))
        a = rng.integers(0, 5, size=na * chunk).astype(np.uint8)
        b = common.mutate(rng, a, sub=0.1, indel=0.05, geo=0.4, alphabet=5) if rng.random() < 0.7 and na else rng.integers(0, 5, size=nb * chunk).astype(np.uint8)
        b = b[:(len(b) // chunk) * chunk]
        alphas.append(a); betas.append(b)
    # one pair of 1400 x 1450 chunk cells (2.0e6): seven strips of the int64 kernel, related sequences
    a = rng.integers(0, 4, size=1400 * chunk).astype(np.uint8)
    b = common.mutate(rng, a, sub=0.05, indel=0.01, geo=0.4, alphabet=4)
    b = np.concatenate([b, rng.integers(0, 4, size=1450 * chunk).astype(np.uint8)])[:1450 * chunk]
    alphas.append(a); betas.append(b)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, x1000, -2400000, -600000)
    sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
    assert int(np.abs(sc).max()) * 4 > 2 ** 31  # the keys really leave int32
    for k, (a, b) in enumerate(zip(alphas, betas)):
        assert _n1_got(sc, ops, off, k) == oracle.affine_gap_chunk(x1000, -2400000, -600000, chunk, a, b), k
    # positive gapOpen (no h-form anywhere) at the same scale
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, x1000, 200000, -600000)
    sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas[:12], betas[:12])
    for k in range(12):
        assert _n1_got(sc, ops, off, k) == oracle.affine_gap_chunk(x1000, 200000, -600000, chunk, alphas[k], betas[k]), ("gapOpen > 0", k)
    # groups (column averages with Go's truncating division, lower case, gaps) with the default matrix x 20 000
    big = [[v * 20000 for v in row] for row in align.DefaultScoreMatrix]
    for ch in (1, 2):
        groups = []
        for _ in range(6):
            nseq, ln = int(rng.integers(1, 5)), int(rng.integers(1, 260)) * ch
            blk = rng.integers(0, 10, size=(nseq, ln)).astype(np.uint8)
            blk[rng.random(blk.shape) < 0.1] = dna.Gap
            blk[0, blk[0] == dna.Gap] = 1
            groups.append(blk)
        pairs = [(x, y) for x in range(len(groups)) for y in range(len(groups)) if x != y]
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, big, -8000000, -600000)
        sc, ops, off = gpu_lib.multiple_affine_gap_batch(p, ch, groups, pairs)
        for k, (x, y) in enumerate(pairs):
            assert _n1_got(sc, ops, off, k) == oracle.multiple_affine_gap(big, -8000000, -600000, ch, groups[x], groups[y]), (ch, x, y)
    # every pair with an empty side, the other one long enough for the int64 route ((nc + mc + 2) * max|penalty| >= 2^27 from 30 cells on)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, x1000, -2400000, -600000)
    for alphas, betas in _all_empty_batches(chunk, 100):
        sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
        assert gpu_lib.get_timing()["fast_path"] == 4
        for k, (a, b) in enumerate(zip(alphas, betas)):
            assert _n1_got(sc, ops, off, k) == oracle.affine_gap_chunk(x1000, -2400000, -600000, chunk, a, b), ("all empty", len(alphas), k)


def test_n1_int64_kernel_forced(gpu_lib, geometry, monkeypatch):
    """GNX_WIDE=2: the ordinary N1 fuzz shapes through the int64 kernel (plain 4 * s score matrices, literal recurrences) -- same answers"""
    if geometry == "general":
        pytest.skip("the int64 kernel has one geometry")
    monkeypatch.setenv("GNX_WIDE", "2")
    rng = np.random.default_rng(8)
    for chunk in (1, 3):
        alphas, betas = [], []
        for _ in range(40):
            na, nb = int(rng.integers(0, 70)), int(rng.integers(0, 90))
            a = rng.integers(0, 5, size=na * chunk).astype(np.uint8)
            b = common.mutate(rng, a, sub=0.1, indel=0.05, geo=0.4, alphabet=5) if rng.random() < 0.6 and na else rng.integers(0, 5, size=nb * chunk).astype(np.uint8)
            b = b[:(len(b) // chunk) * chunk]
            alphas.append(a); betas.append(b)
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, align.HumanChimpTwoScoreMatrix, -600, -150)
        sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
        for k, (a, b) in enumerate(zip(alphas, betas)):
            assert _n1_got(sc, ops, off, k) == oracle.affine_gap_chunk(MX["HumanChimpTwo"], -600, -150, chunk, a, b), (chunk, k)
        for alphas, betas in _all_empty_batches(chunk, 100):  # every pair with an empty side: no fill launch at all
            sc, ops, off = gpu_lib.affine_gap_chunk_batch(p, chunk, alphas, betas)
            assert gpu_lib.get_timing()["fast_path"] == 4
            for k, (a, b) in enumerate(zip(alphas, betas)):
                assert _n1_got(sc, ops, off, k) == oracle.affine_gap_chunk(MX["HumanChimpTwo"], -600, -150, chunk, a, b), ("all empty", chunk, len(alphas), k)
