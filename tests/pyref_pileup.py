"""The specification of gnx_pileup_* (include/gnx_align.h) restated literally: the CIGAR is expanded into a Python list of columns and
every count is bumped column by column; the call rule is applied position by position.  No numpy tricks, no run arithmetic: every GPU
test is equality with this."""
import pyref_summary

M, I, D = 0, 1, 2
LOCAL = 3
SUB, DEL, INS = 0, 1, 2


def new_pile(region_len):
    """one dict per position of the region: base[strand][A C G T N], del[strand], ins[strand]"""
    return [{"base": [[0] * 5, [0] * 5], "del": [0, 0], "ins": [0, 0]} for _ in range(region_len)]


def add(pile, mode, window_start, window, read, strand, route, region):
    """one alignment: `window` (alpha; only its length could matter, and it does not: the CIGAR says what is consumed) at reference
    position window_start, `read` (beta) in the orientation it was aligned in, region = (start, len) of the pile"""
    assert mode == LOCAL and strand in (0, 1)
    del window
    cols = pyref_summary.columns(route)
    lead = 0
    while lead < len(cols) and cols[lead] == D:
        lead += 1
    end = len(cols)
    while end > lead and cols[end - 1] == D:
        end -= 1
    alpha_start = lead
    alpha_end = sum(1 for c in cols[:end] if c != I)  # the alpha bases before the trailing run (one D run as a whole: nothing is inside anyway)
    r_start, r_len = region

    def bump(x, field, slot=None):
        if r_start <= x < r_start + r_len:
            row = pile[x - r_start]
            if slot is None:
                row[field][strand] += 1
            else:
                row[field][strand][slot] += 1

    i = j = 0
    for k, c in enumerate(cols):
        inside = lead <= k < end
        if c == M:
            if inside:
                bump(window_start + i, "base", min(int(read[j]), 4))
            i += 1
            j += 1
        elif c == D:
            if inside:
                bump(window_start + i, "del")
            i += 1
        else:
            starts_run = k == 0 or cols[k - 1] != I  # the first column of a maximal I run
            if inside and starts_run and alpha_start < i < alpha_end:
                bump(window_start + i - 1, "ins")
            j += 1
    return pile


def _passes(opts, depth, count, fwd):
    return (depth >= opts["min_depth"] and count >= opts["min_alt"] and count * opts["frac_den"] >= opts["frac_num"] * depth
            and (not opts["both_strands"] or (fwd >= 1 and count - fwd >= 1)))


def calls(pile, ref_codes, opts, region_start=0):
    """the calls of a pile whose row k lies over reference position region_start + k, ref_codes[k] its code (4: N);
    opts = {"min_depth", "min_alt", "frac_num", "frac_den", "both_strands"}.  -> [(pos, depth, count, count_fwd, kind, ref, alt)]"""
    out = []
    for k, row in enumerate(pile):
        c = int(ref_codes[k])
        if c >= 4:
            continue
        cnt = [row["base"][0][a] + row["base"][1][a] for a in range(5)]
        dele, ins = row["del"][0] + row["del"][1], row["ins"][0] + row["ins"][1]
        depth = sum(cnt) + dele
        cands = [(cnt[a], row["base"][0][a], SUB, a) for a in range(4) if a != c] + [(dele, row["del"][0], DEL, 0xFF)]
        best = cands[0]
        for cand in cands[1:]:
            if cand[0] > best[0]:  # ties go to the earlier candidate
                best = cand
        if _passes(opts, depth, best[0], best[1]):
            out.append((region_start + k, depth, best[0], best[1], best[2], c, best[3]))
        if _passes(opts, depth, ins, row["ins"][0]):
            out.append((region_start + k, depth, ins, row["ins"][0], INS, c, 0xFF))
    return out


def rows(pile):
    """the pile as nested lists in gnx_pile's order: [base[0], base[1], del, ins] per position"""
    return [[list(r["base"][0]), list(r["base"][1]), list(r["del"]), list(r["ins"])] for r in pile]
