"""CPU-side checks of the score-only chunk / multiple-alignment entries (gnx_*_score_batch) and of the score-first progressive
driver: symbols and bindings, errors that need no device (the resources of the sweep's kernels: test_kernel_resources.py),
the driver on the CPU oracle (results, number of engine calls, reuse of remembered scores) and the identity behind that reuse."""
import ctypes
import os
import re

import numpy as np
import pytest

import n1_helpers
import oracle
from gonomics_amd import _lib, align, dna, fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gnx_affine_gap_chunk_score_batch", "gnx_multiple_affine_gap_score_batch"]


def test_n1_score_symbols_exported_and_declared():
    raw = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    L = _lib.lib()
    for nm in ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("affine_gap_chunk_score_batch", "multiple_affine_gap_score_batch"):
        assert callable(getattr(_lib, fn))
    for fn in ("AffineGapChunkScore", "multipleAffineGapScoreBatch"):
        assert callable(getattr(align, fn))
    assert "9" in re.search(r"int32_t fast_path;.*?\*/", raw, flags=re.S).group(0)


def _code(fn, *args):
    with pytest.raises(_lib.GnxError) as ei:
        fn(*args)
    return ei.value.code


def test_n1_score_errors_without_a_device():
    """a bad mode or chunk size is GNX_EINVAL before a device is looked for; a good call without a device is GNX_EDEVICE"""
    L = _lib.lib()
    a, b = dna.StringToBases("ACGTAC"), dna.StringToBases("ACGTTT")
    blocks = [a[None, :], b[None, :]]
    good = _lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, align.DefaultScoreMatrix, -400, -30)
    for mode in (_lib.GNX_AFFINE_GAP, _lib.GNX_CONST_GAP, _lib.GNX_AFFINE_GAP_LOCAL):
        bad = _lib.make_params(mode, align.DefaultScoreMatrix, -400, -30)
        assert _code(_lib.affine_gap_chunk_score_batch, bad, 3, [a], [b]) == _lib.GNX_EINVAL
        assert _code(_lib.multiple_affine_gap_score_batch, bad, 3, blocks, [(0, 1)]) == _lib.GNX_EINVAL
    for chunk in (0, -1):
        assert _code(_lib.affine_gap_chunk_score_batch, good, chunk, [a], [b]) == _lib.GNX_EINVAL
        assert _code(_lib.multiple_affine_gap_score_batch, good, chunk, blocks, [(0, 1)]) == _lib.GNX_EINVAL
    if L.gnx_device_count() > 0:
        return  # (with a GPU the good call is covered by the gpu tests)
    assert _code(_lib.affine_gap_chunk_score_batch, good, 3, [a], [b]) == _lib.GNX_EDEVICE
    assert _code(_lib.multiple_affine_gap_score_batch, good, 3, blocks, [(0, 1)]) == _lib.GNX_EDEVICE
    with pytest.raises(_lib.GnxError) as ei:
        align.AffineGapChunkScore(a, b, align.DefaultScoreMatrix, -400, -30, 3)
    assert ei.value.code == _lib.GNX_EDEVICE


# ---- the score-first driver on the oracle ------------------------------------------------------------------------------------------
def _blocks(groups):
    return [np.stack([np.asarray(f.Seq, dtype=np.uint8) for f in g]) for g in groups]


class _Engines:
    def __init__(self):
        self.score_pairs, self.score_calls, self.align_pairs, self.exchanged = 0, 0, 0, 0
        self.seen = set()

    def _key(self, g):
        return tuple(sorted(f.Name for f in g))

    def score(self, groups, pairs, scores, gapOpen, gapExtend, chunkSize):
        bl = _blocks(groups)
        self.score_calls += 1
        self.score_pairs += len(pairs)
        for x, y in pairs:
            kx, ky = self._key(groups[x]), self._key(groups[y])
            assert (kx, ky) not in self.seen, "a pair was scored twice in the same order"
            self.exchanged += (ky, kx) in self.seen
            self.seen.add((kx, ky))
        return [oracle.multiple_affine_gap(scores, gapOpen, gapExtend, chunkSize, bl[x], bl[y])[0] for x, y in pairs]

    def align(self, groups, pairs, scores, gapOpen, gapExtend, chunkSize):
        bl = _blocks(groups)
        self.align_pairs += len(pairs)
        out = []
        for x, y in pairs:
            s, route = oracle.multiple_affine_gap(scores, gapOpen, gapExtend, chunkSize, bl[x], bl[y])
            out.append((s, [align.Cigar(r, o) for r, o in route]))
        return out


def _record_sets():
    rng = np.random.default_rng(417)
    sets = []
    for G, chunk, alphabet in ((5, 1, 4), (8, 3, 4), (6, 3, 2), (7, 1, 4), (6, 1, 2)):
        recs = []
        for k in range(G):
            ln = int(rng.integers(20, 61)) // chunk * chunk
            recs.append(fasta.Fasta("s%d" % k, rng.integers(0, alphabet, size=max(ln, chunk)).astype(np.uint8)))
        sets.append((recs, chunk))
    recs, chunk = sets[3]
    recs[4] = fasta.Fasta("s4", recs[1].Seq.copy())  # two identical records: their scores against everything tie
    return sets


ASYM = [[91, -114, -31, -123, -44], [-90, 100, -125, -31, -43], [-50, -100, 100, -114, -43], [-123, -31, -80, 91, -43], [-44, -43, -43, -43, -43]]


def _same(got, exp):
    return [(f.Name, bytes(np.asarray(f.Seq, np.uint8))) for f in got] == [(f.Name, bytes(np.asarray(f.Seq, np.uint8))) for f in exp]


def test_score_first_driver_on_the_oracle(monkeypatch):
    monkeypatch.setenv("GNX_N1_SCORE_FIRST", "1")
    for recs, chunk in _record_sets():
        G = len(recs)
        exp = n1_helpers.all_seq_affine_oracle(recs, align.DefaultScoreMatrix, -400, -30, chunk)
        e = _Engines()
        got = align._all_seq(recs, align.DefaultScoreMatrix, -400, -30, chunk, e.align, e.score)
        assert _same(got, exp), (G, chunk)
        assert e.score_pairs == (G - 1) ** 2 and e.align_pairs == G - 1, (G, chunk, e.score_pairs, e.align_pairs)
        assert e.score_calls == G - 1  # one call per round: G(G-1)/2 pairs, then g - 1 per round that begins with g groups
        # a deliberately asymmetric matrix: the same result, and no exchanged pair reuses its score (each is scored again, exchanged)
        exp = n1_helpers.all_seq_affine_oracle(recs, ASYM, -400, -30, chunk)
        e = _Engines()
        got = align._all_seq(recs, ASYM, -400, -30, chunk, e.align, e.score)
        assert _same(got, exp), ("asymmetric", G, chunk)
        assert e.align_pairs == G - 1 and e.score_pairs >= (G - 1) ** 2


def test_asymmetric_matrix_rescans_exchanged_pairs(monkeypatch):
    """the move groups[y] = groups[-1] exchanges sides: with an asymmetric matrix those pairs are scored again, with a symmetric one not"""
    monkeypatch.setenv("GNX_N1_SCORE_FIRST", "1")
    exchanged = 0
    for recs, chunk in _record_sets():
        e = _Engines()
        align._all_seq(recs, ASYM, -400, -30, chunk, e.align, e.score)
        exchanged += e.exchanged
        assert e.score_pairs == (len(recs) - 1) ** 2 + e.exchanged
    assert exchanged > 0  # the sets do exercise the case


@pytest.mark.parametrize("setting", [None, "0"])
def test_score_first_switch_off_is_the_old_driver(monkeypatch, setting):
    """unset (the default, see DESIGN.md 4.17 for the measurement behind it) and 0: every pair with its route, every round"""
    if setting is None:
        monkeypatch.delenv("GNX_N1_SCORE_FIRST", raising=False)
    else:
        monkeypatch.setenv("GNX_N1_SCORE_FIRST", setting)
    recs, chunk = _record_sets()[1]
    G = len(recs)
    e = _Engines()
    got = align._all_seq(recs, align.DefaultScoreMatrix, -400, -30, chunk, e.align, e.score)
    assert _same(got, n1_helpers.all_seq_affine_oracle(recs, align.DefaultScoreMatrix, -400, -30, chunk))
    assert e.score_pairs == 0 and e.align_pairs == sum(g * (g - 1) // 2 for g in range(2, G + 1))


def test_score_first_raises_when_the_engines_disagree(monkeypatch):
    monkeypatch.setenv("GNX_N1_SCORE_FIRST", "1")
    recs, chunk = _record_sets()[0]
    e = _Engines()
    with pytest.raises(RuntimeError):
        align._all_seq(recs, align.DefaultScoreMatrix, -400, -30, chunk, e.align, lambda *a: [s + 1 for s in e.score(*a)])


def test_exchanged_sides_score_the_same_with_the_transposed_matrix():
    """score(A, B, S) == score(B, A, S^T): what lets an exchanged pair reuse its score when S is symmetric"""
    rng = np.random.default_rng(52)
    n = 0
    for chunk in (1, 3):
        for _ in range(30):
            blocks = []
            for _side in range(2):
                nseq, ln = int(rng.integers(1, 4)), int(rng.integers(1, 25)) * chunk
                blk = rng.integers(0, 10, size=(nseq, ln)).astype(np.uint8)  # upper and lower case
                blk[rng.random(blk.shape) < 0.12] = dna.Gap
                blk[0, blk[0] == dna.Gap] = int(rng.integers(0, 4))  # one member without gaps: no gap-only column pair
                blocks.append(blk)
            S = rng.integers(-130, 110, size=(5, 5)).tolist()
            ST = [[S[b][a] for b in range(5)] for a in range(5)]
            go, ge = (-400, -30) if n % 2 else (-7, -3)
            assert oracle.multiple_affine_gap(S, go, ge, chunk, blocks[0], blocks[1])[0] == oracle.multiple_affine_gap(ST, go, ge, chunk, blocks[1], blocks[0])[0]
            n += 1
    assert n >= 50
