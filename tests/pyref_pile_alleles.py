"""The specification of gnx_pileup_alleles / gnx_pileup_indel_calls (include/gnx_align.h) restated literally: the CIGAR is expanded into a
Python list of columns, maximal runs are found by scanning the columns one by one, every allele is a key of a dict of counts, and the
call rule is applied allele by allele.  No run arithmetic: every GPU test is equality with this."""
import pyref_pileup
import pyref_summary

M, I, D = 0, 1, 2
DEL, INS, LONG_INS = 1, 2, 3
SEQ_MAX = 21


def pack(bases):
    """3 bits a base, code + 1 (N: 5), the first base in the lowest bits"""
    v = 0
    for k, b in enumerate(bases):
        v += (min(int(b), 4) + 1) * 8 ** k
    return v


def new_alleles():
    """(pos, kind, key) -> [count on strand 0, count on strand 1]"""
    return {}


def events(window_start, read, route, region):
    """the events of one alignment as (pos, kind, key), in column order"""
    cols = pyref_summary.columns(route)
    lead = 0
    while lead < len(cols) and cols[lead] == D:
        lead += 1
    end = len(cols)
    while end > lead and cols[end - 1] == D:
        end -= 1
    alpha_start = lead
    alpha_end = sum(1 for c in cols[:end] if c != I)
    r_start, r_len = region
    out = []
    i = j = 0
    k = 0
    while k < len(cols):
        c = cols[k]
        if c == M:
            i += 1
            j += 1
            k += 1
            continue
        first = k  # the maximal run of c that starts at column k
        while k < len(cols) and cols[k] == c:
            k += 1
        n = k - first
        if c == D:
            if lead <= first < end and r_start <= window_start + i < r_start + r_len:
                out.append((window_start + i, DEL, n))
            i += n
        else:
            if lead <= first < end and alpha_start < i < alpha_end and r_start <= window_start + i - 1 < r_start + r_len:
                out.append((window_start + i - 1, INS, pack(read[j:j + n])) if n <= SEQ_MAX else (window_start + i - 1, LONG_INS, n))
            j += n
    return out


def add(alleles, window_start, read, strand, route, region):
    for ev in events(window_start, read, route, region):
        alleles.setdefault(ev, [0, 0])[strand] += 1
    return alleles


def listed(alleles):
    """-> [(pos, kind, key, count, count_fwd)], ordered by (pos, kind, key)"""
    return [(pos, kind, key, f + r, f) for (pos, kind, key), (f, r) in sorted(alleles.items())]


def calls(alleles, pile, ref_codes, opts, region_start=0):
    """the indel calls of `alleles` against `pile` (pyref_pileup's, row k over region_start + k; ref_codes[k] its code)
    -> [(pos, kind, key, count, count_fwd, depth, ref)]"""
    out = []
    for pos, kind, key, count, fwd in listed(alleles):
        row = pile[pos - region_start]
        c = int(ref_codes[pos - region_start])
        if c >= 4:
            continue
        depth = sum(row["base"][0]) + sum(row["base"][1]) + row["del"][0] + row["del"][1]
        if pyref_pileup._passes(opts, depth, count, fwd):
            out.append((pos, kind, key, count, fwd, depth, c))
    return out
