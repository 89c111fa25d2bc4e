"""Inputs shared by tests/test_md_cpu.py and tests/test_md_gpu.py: the worked values of the header, the pair whose decimals sit on every
digit boundary, and the long D group.  The seam cases and the random related pairs are summary_cases'."""
import functools

import numpy as np

import summary_cases as sc

M, I, D = sc.M, sc.I, sc.D
ALPHA = "ACGTACGTAC"
# (mode, beta, route, MD) on alpha = ALPHA: the table of include/gnx_align.h's contract
WORKED = [(2, "ACGAACTAC", [(6, M), (1, D), (3, M)], "3T2^G3"),
          (3, "TTTACG", [(3, D), (2, I), (4, M), (3, D)], "4"),
          (0, "TTTACG", [(3, D), (2, I), (4, M), (3, D)], "0^ACG4^TAC0"),
          (3, "", [(4, D), (0, M), (3, D)], "0"),
          (4, "", [(4, D), (0, M), (3, D)], "0^ACGTACG0")]
M63_64_65 = "62C0A62G0^A65"
# the pinned values of gnx_mapq_batch: (score, second score or None, MAPQ)
MAPQ_PINS = [(0, None, 0), (-5, 3, 0), (400, None, 60), (400, -40, 60), (400, 400, 0), (400, 500, 0), (400, 399, 0), (400, 200, 30), (400, 1, 59), (61, 1, 59),
             (1 << 62, 1 << 61, 30)]

STRETCHES = (9, 10, 99, 100, 999, 1000, 9999)


@functools.lru_cache(maxsize=None)
def digit_boundary():
    """(alpha, beta, route): the equal stretches are exactly STRETCHES, in that order, with one substitution between two of them.  Run
    boundaries: a zero-length D run at column 150 (inside the stretch of 100), M | M seams at columns 640 and 1280 (multiples of 64, inside
    the stretches of 999 and 1 000), an I run of two at column 5 000 (inside the stretch of 9 999)."""
    rng = np.random.default_rng(101)
    n = sum(STRETCHES) + len(STRETCHES) - 1
    alpha = rng.integers(0, 4, size=n).astype(np.uint8)
    same = alpha.copy()
    at, subs = 0, []
    for s in STRETCHES[:-1]:
        at += s
        same[at] = (same[at] + 1 + int(rng.integers(0, 3))) % 4
        subs.append(at)
        at += 1
    assert (150, 640, 1280) == (150, 64 * 10, 64 * 20) and subs[3] < 640 < subs[4] < 1280 < subs[5] < 5000 and subs[2] < 150 < subs[3]
    beta = np.concatenate([same[:5000], rng.integers(0, 4, size=2).astype(np.uint8), same[5000:]])
    route = [(150, M), (0, D), (490, M), (640, M), (3720, M), (2, I), (n - 5000, M)]
    return alpha, beta, route


def digit_boundary_md():
    """what that pair's MD must look like, from its construction alone"""
    alpha, _, _ = digit_boundary()
    out, at = [], 0
    for s in STRETCHES[:-1]:
        at += s
        out.append("%d%s" % (s, "ACGT"[int(alpha[at])]))
        at += 1
    return "".join(out) + "%d" % STRETCHES[-1]


@functools.lru_cache(maxsize=None)
def d_group():
    """(alpha, beta, route): a D group of 200 columns given as 70 runs of one and one run of 130, between two M runs -- it straddles a
    block of 64 runs, and its last run takes the lane-per-column form"""
    rng = np.random.default_rng(102)
    route = [(5, M)] + [(1, D)] * 70 + [(130, D)] + [(7, M)]
    alpha, beta = sc._fit(rng, route, equal=0.7)
    return alpha, beta, route


def batch_with(extra):
    """(names, alphas, betas, routes): `extra` = [(name, alpha, beta, route)] in the middle of three short seam cases"""
    short = [c for c in sc.seam_cases() if c[0] in ("m63_64_65", "same_op_adjacent", "lead_and_trail_d")]
    cases = short[:2] + list(extra) + short[2:]
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]
