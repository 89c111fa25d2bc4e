"""The selection rule of gnx_best_pair_* restated in plain Python: the specification the tests compare the device against.

A candidate is (score, A, E, strand): its local-alignment score, the absolute start and end of the alignment on the target
(A = window start + span start, E = window start + span end) and the strand of the read it was scored with."""
INT64_MIN = -(1 << 63)


def first_max(scores):
    """index of the first maximum, -1 for an empty list (gnx_best_of_*'s rule)"""
    best = -1
    for k, s in enumerate(scores):
        if best < 0 or s > scores[best]:
            best = k
    return best


def insert(c1, c2, min_insert, max_insert):
    """E(v) - A(f) if the combination is proper, else None"""
    if c1[3] == c2[3] or c1[2] <= c1[1] or c2[2] <= c2[1]:
        return None
    f, v = (c1, c2) if c1[3] == 0 else (c2, c1)
    if f[1] > v[1] or f[2] > v[2]:
        return None
    t = v[2] - f[1]
    return t if min_insert <= t <= max_insert else None


def second(cands, chosen):
    rest = [c[0] for k, c in enumerate(cands) if k != chosen]
    return max(rest) if rest else INT64_MIN


def select(mate1, mate2, min_insert, max_insert, unpaired_penalty):
    """((best1, best2), proper, tlen, (second1, second2)) of one read pair"""
    top = None
    for x, c1 in enumerate(mate1):
        for y, c2 in enumerate(mate2):
            t = insert(c1, c2, min_insert, max_insert)
            if t is not None and (top is None or c1[0] + c2[0] > top[0]):  # (x, y) ascend: ties stay with the lowest c1, then c2
                top = (c1[0] + c2[0], x, y, t)
    b1, b2 = first_max([c[0] for c in mate1]), first_max([c[0] for c in mate2])
    if top is not None and top[0] >= mate1[b1][0] + mate2[b2][0] - unpaired_penalty:
        return (top[1], top[2]), 1, top[3], (second(mate1, top[1]), second(mate2, top[2]))
    return (b1, b2), 0, 0, (second(mate1, b1), second(mate2, b2))


def select_all(per_read, min_insert, max_insert, unpaired_penalty):
    """per_read[r] = the candidates of read r, reads 2k and 2k + 1 mates.  Returns (best, second) per read and (proper, tlen) per pair."""
    best, sec, proper, tlen = [], [], [], []
    for k in range(len(per_read) // 2):
        b, p, t, s = select(per_read[2 * k], per_read[2 * k + 1], min_insert, max_insert, unpaired_penalty)
        best += list(b); sec += list(s); proper.append(p); tlen.append(t)
    return best, sec, proper, tlen
