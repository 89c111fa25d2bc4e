"""CPU-side checks of the score-only entries (gnx_score_*): symbols and bindings, the no-device error, the selection rule of
AlignBestOf with stub score / align functions.  The resources of the sweep's kernels: test_kernel_resources.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_ENTRIES = ["gnx_score_batch", "gnx_score_batch_windows", "gnx_score_batch_by_offset", "gnx_score_batch_device"]


def test_score_symbols_exported_and_declared():
    hdr = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    L = _lib.lib()
    for nm in SCORE_ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("score_batch", "score_batch_windows", "score_batch_by_offset"):
        assert callable(getattr(_lib, fn))
    for fn in ("ScoreBatch", "AffineGapScore", "ConstGapScore", "AffineGapLocalScore", "ScoreAllPairs", "AlignBestOf"):
        assert callable(getattr(align, fn))
    assert "7" in re.search(r"int32_t fast_path;.*?\*/", open(os.path.join(ROOT, "include", "gnx_align.h")).read(), flags=re.S).group(0)


def test_score_without_a_device_is_an_error():
    L = _lib.lib()
    if L.gnx_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    with pytest.raises(_lib.GnxError) as ei:
        align.AffineGapScore(dna.StringToBases("ACGT"), dna.StringToBases("ACG"), align.DefaultScoreMatrix, -400, -30)
    assert ei.value.code == _lib.GNX_EDEVICE
    with pytest.raises(_lib.GnxError) as ei:
        align.ScoreAllPairs([dna.StringToBases("ACGT"), dna.StringToBases("ACG"), dna.StringToBases("AC")], _lib.make_params(_lib.GNX_CONST_GAP, align.DefaultScoreMatrix, -400))
    assert ei.value.code == _lib.GNX_EDEVICE


def test_score_device_entry_without_a_device_is_an_error():
    L = _lib.lib()
    if L.gnx_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    assert callable(_lib.score_batch_device) and callable(_lib.align_batch_device)
    for mode in range(5):
        p = _lib.make_params(mode, align.DefaultScoreMatrix, -400, -30 if mode in (0, 2, 3) else 0)
        assert _lib.score_batch_device(p, 2, 0, 0, 0, 0, np.asarray([3, 4], np.int64), np.asarray([5, 6], np.int64), 0) == _lib.GNX_EDEVICE


def test_align_best_of_selection_rule(monkeypatch):
    """first maximum in candidate order, ties to the lowest index, K_r varying, K_r = 1 -- with stub score and align functions"""
    table = {}  # (read id, candidate id) -> score; a sequence's id is its first element
    calls = {"score": 0, "align": 0}

    def fake_score(params, alphas, betas):
        calls["score"] += 1
        return np.asarray([table[(int(a[0]), int(b[0]))] for a, b in zip(alphas, betas)], dtype=np.int64)

    def fake_align(params, alphas, betas):
        calls["align"] += 1
        sc = np.asarray([table[(int(a[0]), int(b[0]))] for a, b in zip(alphas, betas)], dtype=np.int64)
        ops = np.zeros(len(alphas), dtype=_lib.CIGAR_DTYPE)
        ops["run_length"] = [int(b[0]) for b in betas]  # the route names the candidate it was computed for
        return sc, ops, np.arange(len(alphas) + 1, dtype=np.int64)

    monkeypatch.setattr(_lib, "score_batch", fake_score)
    monkeypatch.setattr(_lib, "align_batch", fake_align)
    reads = [np.asarray([r, 0, 1], dtype=np.uint8) for r in range(5)]
    per_read = [[5, 9, 9, 3], [7], [-4, -4, -4], [1, 2, 3, 4, 5, 6], [8, 2, 8]]  # K_r = 4, 1, 3, 6, 3
    want = [1, 0, 0, 5, 0]
    cands, cid = [], 10
    for r, row in enumerate(per_read):
        cs = []
        for s in row:
            table[(r, cid)] = s
            cs.append(np.asarray([cid, 2, 3], dtype=np.uint8))
            cid += 1
        cands.append(cs)
    got = align.AlignBestOf(_lib.make_params(_lib.GNX_AFFINE_GAP, align.DefaultScoreMatrix, -400, -30), reads, cands)
    assert calls == {"score": 1, "align": 1}
    assert [g[0] for g in got] == want
    for r, (b, s, route) in enumerate(got):
        assert s == per_read[r][want[r]]
        assert route == [align.Cigar(int(cands[r][b][0]), 0)]  # the align call saw the winner, nothing else
    assert align._first_maxima([3, 3, 1, 2, 2], [3, 2]) == [0, 0]
    with pytest.raises(ValueError):
        align._first_maxima([1], [1, 0])
    assert align.AlignBestOf(None, [], []) == []
