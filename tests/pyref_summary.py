"""The specification of gnx_summarize_* (include/gnx_align.h) restated literally: the CIGAR is expanded into a Python list of columns
and every field is computed from that list.  No numpy tricks, no run arithmetic: every GPU test is equality with this."""

M, I, D, EQ, X = 0, 1, 2, 3, 4
AFFINE_MODES = (0, 2, 3)
LOCAL = 3
FIELDS = ("rescore", "alpha_used", "beta_used", "alpha_start", "alpha_end", "n_equal", "n_mismatch", "ins_bases", "del_bases", "gap_runs", "n_xops")


def columns(route):
    """the column sequence: runs of length 0 contribute nothing"""
    cols = []
    for run, op in route:
        cols.extend([int(op)] * int(run))
    return cols


def _runs(types):
    out = []
    for t in types:
        if out and out[-1][1] == t:
            out[-1][0] += 1
        else:
            out.append([1, t])
    return [(n, t) for n, t in out]


def summarize(mode, scores, gap_open, gap_extend, alpha, beta, route):
    """(summary dict, extended CIGAR as [(run, type), ...]); scores = 5 x 5 or 25 flat; route = [(run_length, op), ...]"""
    flat = [int(v) for row in scores for v in row] if len(scores) == 5 else [int(v) for v in scores]
    cols = columns(route)
    i = j = 0
    types, match = [], 0
    for c in cols:
        if c == M:
            a, b = int(alpha[i]), int(beta[j])
            types.append(EQ if a == b else X)
            match += flat[a * 5 + b]
            i += 1
            j += 1
        elif c == I:
            types.append(I)
            j += 1
        else:
            types.append(D)
            i += 1
    free = [False] * len(cols)
    lead = trail = 0
    if mode == LOCAL:
        while lead < len(cols) and cols[lead] == D:
            free[lead] = True
            lead += 1
        k = len(cols)
        while k > lead and cols[k - 1] == D:
            k -= 1
            free[k] = True
            trail += 1
    charged = [c for c, f in zip(cols, free) if not f]
    ins, dele = charged.count(I), charged.count(D)
    gap_runs = sum(1 for _, t in _runs(charged) if t in (I, D))
    if mode == LOCAL and cols and lead == len(cols):
        a_start = a_end = 0
    elif mode == LOCAL:
        a_start, a_end = lead, i - trail
    else:
        a_start, a_end = 0, i
    if mode in AFFINE_MODES:
        rescore = match + gap_open * gap_runs + gap_extend * (ins + dele)
    else:
        rescore = match + gap_open * (ins + dele)
    x = _runs(types)
    s = {"rescore": rescore, "alpha_used": i, "beta_used": j, "alpha_start": a_start, "alpha_end": a_end, "n_equal": types.count(EQ), "n_mismatch": types.count(X),
         "ins_bases": ins, "del_bases": dele, "gap_runs": gap_runs, "n_xops": len(x)}
    return s, x
