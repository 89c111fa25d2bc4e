"""The specification of the quality pile and of gnx_pileup_genotypes (include/gnx_align.h) restated literally: the CIGAR is expanded into
a Python list of columns, every count and every quality sum is bumped column by column, and the genotype rule is applied position by
position with Python's unbounded integers.  Every GPU test of tests/test_pile_qual_gpu.py is equality with this."""
import pyref_pileup
import pyref_summary

M, I, D = pyref_pileup.M, pyref_pileup.I, pyref_pileup.D
LOCAL = pyref_pileup.LOCAL
QUAL_MAX = 93
SAT = 2 ** 31 - 1


def new_pile(region_len):
    """pyref_pileup's rows with qsum[A C G T] beside them"""
    pile = pyref_pileup.new_pile(region_len)
    for row in pile:
        row["qsum"] = [0] * 4
    return pile


def add(pile, mode, window_start, read, quals, strand, route, region, min_baseq):
    """one alignment with its qualities (raw Phred bytes, one per read base, in the read's orientation)"""
    assert mode == LOCAL and strand in (0, 1) and len(quals) == len(read)
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
    i = j = 0
    for k, c in enumerate(cols):
        inside = lead <= k < end
        x = window_start + i
        if c == M:
            if inside and r_start <= x < r_start + r_len:
                b, q = min(int(read[j]), 4), min(int(quals[j]), QUAL_MAX)
                if q >= min_baseq:
                    pile[x - r_start]["base"][strand][b] += 1
                    if b < 4:
                        pile[x - r_start]["qsum"][b] += q
            i += 1
            j += 1
        elif c == D:
            if inside and r_start <= x < r_start + r_len:
                pile[x - r_start]["del"][strand] += 1
            i += 1
        else:
            starts_run = k == 0 or cols[k - 1] != I
            if inside and starts_run and alpha_start < i < alpha_end and r_start <= x - 1 < r_start + r_len:
                pile[x - 1 - r_start]["ins"][strand] += 1
            j += 1
    return pile


def opts(min_depth=1, min_qual=0, prior_het=3000, prior_hom=3300):
    return {"min_depth": min_depth, "min_qual": min_qual, "prior_het": prior_het, "prior_hom": prior_hom}


def costs(n, Q, c, o):
    """(b, [L0, L1, L2]) at a position with counts n[A C G T], quality sums Q and reference code c < 4"""
    E = [100 * Q[a] + 477 * n[a] for a in range(4)]
    b = None
    for a in range(4):
        if a != c and (b is None or E[a] > E[b]):  # ties go to the smaller index
            b = a
    return b, [E[b], 301 * (n[c] + n[b]) + o["prior_het"], E[c] + o["prior_hom"]]


def genotype(fwd, rev, Q, c, o):
    """the record of one position, or None: a dict with pl, gq, qual, depth, ref_count, alt_count, alt_fwd, gt, ref, alt"""
    if c >= 4:
        return None
    n = [fwd[a] + rev[a] for a in range(4)]
    depth = sum(n)
    b, L = costs(n, Q, c, o)
    g = 0
    for k in (1, 2):
        if L[k] < L[g]:  # ties go to the smaller index
            g = k
    pl = [min(L[k] - L[g], SAT) for k in range(3)]
    gq = min(pl[k] for k in range(3) if k != g)
    qual = min(max(0, L[0] - min(L[1], L[2])), SAT)
    if depth < o["min_depth"] or g == 0 or qual < o["min_qual"]:
        return None
    return {"gt": g, "ref": c, "alt": b, "pl": pl, "gq": gq, "qual": qual, "depth": min(depth, SAT), "ref_count": min(n[c], SAT), "alt_count": min(n[b], SAT), "alt_fwd": fwd[b]}


def genotypes(pile, ref_codes, o, region_start=0):
    """the records of a pile whose row k lies over reference position region_start + k, ref_codes[k] its code (4: N), ordered by position"""
    out = []
    for k, row in enumerate(pile):
        rec = genotype(row["base"][0][:4], row["base"][1][:4], row["qsum"], int(ref_codes[k]), o)
        if rec is not None:
            out.append(dict(rec, pos=region_start + k))
    return out


def rows(pile):
    """(the count rows as pyref_pileup.rows gives them, the qsum rows)"""
    return pyref_pileup.rows(pile), [list(r["qsum"]) for r in pile]
