"""Plain-Python restatement of gnx_reference_index_build and gnx_seed_candidates (include/gnx_align.h): the whole contract with a
dict, no device.  Bases are dna.Base bytes (A C G T = 0 .. 3, N = 4, anything >= 5 is no base)."""


def codes(x, k):
    """codes(x, k)[q] = dnaToNumber (genomeGraph/align.go:170) of x[q : q + k] -- the 2-bit code, first base most significant -- or
    None when one of its bases is not A C G T"""
    out, v, bad, mask = [], 0, -1, (1 << (2 * k)) - 1
    for i, b in enumerate(x):
        b = int(b)
        if b > 3:
            bad = i
        v = ((v << 2) | (b & 3)) & mask
        if i >= k - 1:
            out.append(v if bad <= i - k else None)
    return out


def index(ref, k, step):
    """[(key, position), ...] sorted by key, equal keys in ascending position"""
    cs = codes(ref, k)
    return sorted((cs[p], p) for p in range(0, len(ref) - k + 1, step) if cs[p] is not None)


def lookup_table(idx):
    table = {}
    for key, pos in idx:
        table.setdefault(key, []).append(pos)
    return table


def revcomp(read):
    return [3 - int(b) if int(b) < 4 else int(b) for b in reversed(read)]


def candidates(ref_len, table, k, read, max_occ, bin, pad, max_cand, min_votes):
    """[(start, len, strand, votes), ...] of one read in the contract's order"""
    n = len(read)
    votes = {}
    for s, x in ((0, [int(b) for b in read]), (1, revcomp(read))):
        for q, c in enumerate(codes(x, k)):
            hits = table.get(c, ()) if c is not None else ()
            if not hits or len(hits) > max_occ:
                continue
            for t in hits:
                b = (t - q) // bin  # Python's // floors
                votes[(s, b)] = votes.get((s, b), 0) + 1
    order = sorted((-v, s, b) for (s, b), v in votes.items() if v >= min_votes)[:max_cand]
    out = []
    for v, s, b in order:
        start = min(max(b * bin - pad, 0), ref_len)
        end = min(max((b + 1) * bin + n + pad, 0), ref_len)
        out.append((start, end - start, s, -v))
    return out


def candidates_batch(ref, k, step, reads, max_occ, bin, pad, max_cand, min_votes):
    table = lookup_table(index(ref, k, step))
    return [candidates(len(ref), table, k, r, max_occ, bin, pad, max_cand, min_votes) for r in reads]
