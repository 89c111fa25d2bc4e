"""Helpers of the span tests (gnx_locate_span_*): what the oracle's CIGAR says about an alignment's target span, the
window bound `lo` of the lemma, and a scalar model of the stage-2 recurrence as span_origin_kernel has it (window, origins, tie
selects, corner, sentinels, strip hand-over)."""
import numpy as np

import oracle

MODE_LOCAL = 3
SENT = -(1 << 30)
FLAT = [[1 if a == b else -1 for b in range(5)] for a in range(5)]
PENALTIES = [(-400, -30), (0, -30), (-7, -3), (-600, -150), (0, -1), (-400, -1)]


def all_matrices():
    import common
    m = dict(common.matrices())
    m["Flat"] = FLAT
    return m


def spans_from_oracle(scores, gap_open, gap_extend, targets, queries, threads=4):
    """(score, start, end) int64 arrays: start = the leading ColD run of the oracle's CIGAR (0 if it does not begin with one, and 0 for a
    CIGAR that is a single ColD run), end = len(target) minus its trailing ColD run."""
    sc, ops, off = oracle.align_batch(MODE_LOCAL, scores, gap_open, gap_extend, targets, queries, threads=threads)
    n = len(targets)
    start = np.zeros(n, dtype=np.int64)
    end = np.zeros(n, dtype=np.int64)
    for p in range(n):
        a, b = int(off[p]), int(off[p + 1])
        e = len(targets[p])
        s = 0
        if b > a:
            if ops["op"][b - 1] == 2:
                e -= int(ops["run_length"][b - 1])
            if ops["op"][a] == 2 and b - a > 1:
                s = int(ops["run_length"][a])
        start[p], end[p] = s, e
    return np.asarray(sc, dtype=np.int64), start, end


def window_lo(S, end, m, scores, gap_open, gap_extend):
    """The lemma's bound: no route that ends at `end` with score S starts left of lo."""
    if gap_extend >= 0:
        return 0
    smaxp = max(0, int(np.max(np.asarray(scores))))
    num = m * smaxp + gap_open - int(S)
    dmax = num // (-gap_extend) if num > 0 else 0
    return max(0, int(end) - m - dmax)


def _pick(a, oa, b, ob, c, oc):
    best, org = a, oa
    if b > best:
        best, org = b, ob
    if c > best:
        best, org = c, oc
    return best, org


def model_span(target, query, scores, gap_open, gap_extend, S, end, strip=192):
    """The kernel's stage 2 for one pair, scalar: returns (start, score of the window DP, lo).  `strip` = query columns per strip
    (the kernel: 64 lanes x 3 columns; how a strip's columns are dealt to lanes does not change what a cell reads)."""
    sc = np.asarray(scores, dtype=np.int64).reshape(5, 5)
    m = len(query)
    o, e = int(gap_open), int(gap_extend)
    oe = o + e
    lo = window_lo(S, end, m, scores, o, e)
    W = int(end) - lo
    # the hand-over rows: the six values of the strip's last column at every window row (in place, like the kernel)
    hand = [[0] * (W + 1) for _ in range(6)]
    strips = (m + strip - 1) // strip
    last = None
    for s in range(strips):
        base = s * strip
        nl = min(strip, m - base)
        more = s + 1 < strips
        # row 0 of the columns base .. base + nl: (M, I, D, oM, oI, oD)
        def row0(j):
            return [0, o, 0, 0, 0, 0] if j == 0 else [SENT, o + j * e, SENT, 0, 0, 0]
        up = [row0(base + l + 1) for l in range(nl)]       # each column at the row above
        diag0 = row0(base)                                   # column `base` at the row above (lane 0's diagonal)
        for i in range(1, W + 1):
            if s == 0:
                left = [SENT, SENT, 0, 0, 0, i]              # column 0: D = 0 leaves from its own row
            else:
                left = [hand[x][i] for x in range(6)]
            first_left = left
            diag = diag0
            tb = min(int(target[lo + i - 1]), 4)
            for l in range(nl):
                u = up[l]
                qb = min(int(query[base + l]), 4)
                nM, onM = _pick(diag[0], diag[3], diag[1], diag[4], diag[2], diag[5])
                nM += int(sc[tb, qb])
                nI, onI = _pick(left[0] + oe, left[3], left[1] + e, left[4], left[2] + oe, left[5])
                nD, onD = _pick(u[0] + oe, u[3], u[1] + oe, u[4], u[2] + e, u[5])
                diag = u                                     # the next column's diagonal: this column at the row above
                left = [nM, nI, nD, onM, onI, onD]
                up[l] = left
            diag0 = first_left
            if more:
                for x in range(6):
                    hand[x][i] = up[nl - 1][x]
        last = up[nl - 1]
    take_m = last[0] >= last[1]
    return lo + (last[3] if take_m else last[4]), (last[0] if take_m else last[1]), lo
