"""Inputs shared by tests/test_summary_cpu.py and tests/test_summary_gpu.py: random related pairs for every mode, and the hand-made
CIGARs that sit on the seams of aln_summary_kernel (64 columns per step, 64 runs per block, zero-length runs, free end gaps)."""
import functools

import numpy as np

import asym
import common
from gonomics_amd import align

M, I, D = 0, 1, 2
MODES = (0, 1, 2, 3, 4)
LOCAL = 3
# (name, matrix, gapOpen, gapExtend); the constant-gap modes take gapOpen as their penalty (HoxD55: its gapExtend, gapOpen being 0)
SCORING = [("HumanChimpTwo", align.HumanChimpTwoScoreMatrix, -600, -150), ("HoxD55", align.HoxD55ScoreMatrix, 0, -70), ("ASYM", asym.ASYM, -400, -30)]


def pens(mode, go, ge):
    if mode in (1, 4):
        return (go if go else ge), 0
    return go, ge


@functools.lru_cache(maxsize=None)
def related_pairs(mode, seed, count, max_len):
    """count (alpha, beta) pairs of 1 .. max_len bases: beta a mutated copy of alpha; N in a fifth of the reads; in local mode alpha is
    the target -- the mutated copy between random flanks -- and beta the query"""
    rng = np.random.default_rng(seed)
    alphas, betas = [], []
    for _ in range(count):
        n = int(rng.integers(1, max_len + 1))
        alphabet = 5 if rng.random() < 0.2 else 4
        a = rng.integers(0, alphabet, size=n).astype(np.uint8)
        b = common.mutate(rng, a, sub=0.08, indel=0.06, geo=0.4, alphabet=alphabet)[:max_len]
        if mode == LOCAL:
            flanks = [rng.integers(0, 4, size=int(rng.integers(0, max_len // 2 + 1))).astype(np.uint8) for _ in range(2)]
            alphas.append(np.concatenate([flanks[0], b, flanks[1]]))
            betas.append(a)
        else:
            alphas.append(a)
            betas.append(b)
    return alphas, betas


def score_is_pinned(mode, alpha, beta, ci, cj):
    """where the column re-score of the reference's CIGAR equals its score: the high-memory modes always, the low-memory ones while the
    pair fits one checkerboard tile (beyond it quirks Q1 / Q2 can make the CIGAR differ from the scored path)"""
    return mode in (2, 3, 4) or (len(alpha) <= ci and len(beta) <= cj)


def _like(rng, a, mismatch_at=()):
    b = np.array(a, dtype=np.uint8)
    for k in mismatch_at:
        b[k] = (b[k] + 1 + int(rng.integers(0, 3))) % 4
    return b


def _fit(rng, route, equal=0.8):
    """sequences for a route: alpha random, beta equal to alpha on `equal` of the M columns; two spare bases behind each"""
    n = sum(r for r, o in route if o != I) + 2
    m = sum(r for r, o in route if o != D) + 2
    a = rng.integers(0, 4, size=n).astype(np.uint8)
    b = rng.integers(0, 4, size=m).astype(np.uint8)
    i = j = 0
    for r, o in route:
        if o == M:
            keep = rng.random(r) < equal
            b[j:j + r] = np.where(keep, a[i:i + r], (a[i:i + r] + 1) % 4)
        i += r if o != I else 0
        j += r if o != D else 0
    return a, b


@functools.lru_cache(maxsize=None)
def seam_cases():
    """[(name, alpha, beta, route)]: every case is run in all five modes"""
    rng = np.random.default_rng(77)
    out = []
    a = rng.integers(0, 4, size=5000).astype(np.uint8)
    out.append(("m5000", a, _like(rng, a, [0, 62, 63, 64, 65, 127, 128, 4999] + list(range(1000, 1070))), [(5000, M)]))
    route = [(63, M), (1, I), (64, M), (1, D), (65, M)]
    a, b = _fit(rng, route, equal=1.0)
    b[62] = (b[62] + 1) % 4      # the last column of the first run
    b[64] = (b[64] + 1) % 4      # the first column of the second (behind the I column)
    b[64 + 63] = (b[64 + 63] + 1) % 4
    out.append(("m63_64_65", a, b, route))
    for runs in (64, 65, 128, 129, 1000):
        route = [(int(rng.integers(1, 4)), int(rng.integers(0, 3))) for _ in range(runs)]
        out.append(("runs%d" % runs,) + _fit(rng, route) + (route,))
    a = rng.integers(0, 4, size=12).astype(np.uint8)
    same, diff = _like(rng, a), _like(rng, a, [3])
    out.append(("zero_at_start", a, same, [(0, M), (0, D), (5, M)]))
    out.append(("zero_at_end", a, same, [(5, M), (0, I), (0, M)]))
    out.append(("zero_between_equal_seam", a, same, [(3, M), (0, D), (3, M)]))
    out.append(("zero_between_different_seam", a, diff, [(3, M), (0, I), (3, M)]))
    out.append(("zero_between_d_runs", a, same[2:], [(2, D), (0, I), (3, D), (4, M)]))
    out.append(("same_op_adjacent", a, diff, [(2, M), (3, M), (1, I), (2, I), (4, M), (1, D), (1, D)]))
    out.append(("empty_cigar", a, same, []))
    out.append(("consumes_less", a, diff[:9], [(4, M)]))
    out.append(("only_zero_runs", a, same, [(0, M), (0, I), (0, D)]))
    # the free end gaps of the mapping mode (charged like any gap in the others)
    out.append(("d_only", a, np.zeros(0, np.uint8), [(7, D)]))
    out.append(("d_only_in_pieces", a, np.zeros(0, np.uint8), [(3, D), (0, M), (4, D)]))
    out.append(("lead_and_trail_d", a, same[3:], [(3, D), (5, M), (4, D)]))
    out.append(("lead_d_then_i", a, np.concatenate([[1, 2], a[3:]]).astype(np.uint8), [(3, D), (2, I), (5, M)]))
    out.append(("i_then_trail_d", a, np.concatenate([a[:5], [0, 3]]).astype(np.uint8), [(5, M), (2, I), (3, D)]))
    lead = [(1, D)] * 70
    route = lead + [(0, I)] * 3 + [(70, M)] + [(0, M)] * 70 + [(1, D)] * 66  # end gaps longer than one block of runs
    out.append(("long_end_gaps",) + _fit(rng, route) + (route,))
    return out
