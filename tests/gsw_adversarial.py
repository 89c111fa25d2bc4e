"""Test infrastructure: ONE adversarial graph and read set for the graph aligner's seed path (tests/test_seed_adversarial.py), built for
the situations that random nodes and 3 %-error reads (test_gsw_reads.make_case) almost never produce: keys with > 100 locations
(homopolymers, 2- and 4-base repeats), match runs that cross one and two 64-bit words, left extensions that stop at the read start or
run into the rainbow's leading 'A's, node and read lengths on and next to multiples of 32, an N as the first / last base of a word,
nodes shorter than the seed (zero index slots) in a chain whose k-mers cross node borders, empty and 1-base reads, reads whose reverse
strand is the repeat, and a read whose N packs to the node's own bits (the two-bit N quirk).  Everything derives from one seeded
generator; expected values come from the restatement tests/pyref_gsw.py alone and are computed once per (seed_len, step)."""
import functools

import numpy as np

import pyref_gsw as ref

SETTINGS = ((2, 5), (8, 1), (16, 1), (31, 3), (32, 1), (32, 32))
N_SPILL_READ = -1  # (index into reads: the last one)


def _with_n(s, ps):
    s = s.copy()
    for p in ps:
        s[p] = 4
    return s


@functools.lru_cache(maxsize=None)
def case():
    """-> (node sequences, edges, reads, (position of the N in the N-spill read)); checked by tripwire() on first use"""
    rng = np.random.default_rng(1)

    def R(n):
        return rng.integers(0, 4, size=n).astype(np.uint8)

    def A(n):
        return np.zeros(n, np.uint8)

    def T(n):
        return np.full(n, 3, np.uint8)

    unit4 = np.tile(np.asarray([0, 1, 2, 3], np.uint8), 40)
    unit2 = np.tile(np.asarray([0, 1], np.uint8), 50)
    rnd = R(200)
    seqs = [A(64), A(96), A(33), unit4, unit2,                                               # 0-4: homopolymers and short-period repeats
            R(32), R(31), R(16), R(15), R(1), _with_n(R(70), [0]),                           # 5-10: the chain (lengths 32 / 31 / 16 / 15 / 1 / N first)
            _with_n(R(70), [31]), _with_n(R(70), [32]), _with_n(R(70), [69]),                # 11-13: an N at the end / start of a word, at the node's end
            np.concatenate([A(40), rnd[:60]]), rnd, np.concatenate([rnd[100:], A(5)]),       # 14-16: shared stretches behind / in front of 'A's
            R(64), R(65), _with_n(R(64), [63]), _with_n(R(96), [32, 64]),                    # 17-20: whole words, one base more, N at word borders
            T(40), T(64)]                                                                    # 21-22: poly-T (the minus strand of poly-A reads and vice versa)
    edges = [(5, 6), (6, 7), (7, 8), (8, 9), (9, 10), (15, 16), (0, 1), (17, 18), (21, 22)]
    reads = [A(16), A(32), A(33), A(64), A(100), unit4[:50], unit4[1:66], unit2[:33], R(15), R(16),
             seqs[5].copy(), seqs[6].copy(), seqs[7].copy(), np.concatenate([seqs[5], seqs[6]]),
             np.concatenate([seqs[6][10:], seqs[7], seqs[8], seqs[9], seqs[10][:30]]),      # spans five chain nodes
             _with_n(rnd[:80], [0]), _with_n(rnd[:80], [31]), _with_n(rnd[:80], [32]), _with_n(rnd[:80], [79]), _with_n(rnd[20:100], [16]),
             np.concatenate([A(40), rnd[:60]]), np.concatenate([A(7), rnd[:60]]),            # (7 leading 'A's: they collide with the rainbow's padding)
             rnd[:64].copy(), rnd[:65].copy(), rnd[3:35].copy(), rnd[31:95].copy(),
             np.concatenate([rnd[150:], rnd[100:140]]), T(50), T(104), seqs[17].copy(), np.concatenate([seqs[17][40:], seqs[18][:40]]),
             np.zeros(0, np.uint8), R(1)]
    # the N-spill quirk: BasesToUint64LeftAln does `answer<<2 | base`, so (A, N) = (0 << 2 | 4) packs to the bits of (C, A).  A copy of
    # a stretch of `rnd` with C A -> A N, both bases inside one word of node 15 (= rnd), has the node's words: matches run across the N.
    p = next(k for k in range(40, 150) if rnd[k] == 1 and rnd[k + 1] == 0 and k % 32 != 31)
    lo = p - 30
    spill = rnd[lo:lo + 64].copy()
    spill[p - lo], spill[p + 1 - lo] = 0, 4
    reads.append(spill)
    return seqs, edges, reads, p + 1 - lo


@functools.lru_cache(maxsize=None)
def ref_graph():
    seqs, edges, _, _ = case()
    return ref.make_graph(seqs, edges)


@functools.lru_cache(maxsize=None)
def ref_reads():
    return [ref.make_read(rd) for rd in case()[2]]


@functools.lru_cache(maxsize=None)
def ref_index(seed_len, step):
    return ref.index_genome(ref_graph(), seed_len, step)


@functools.lru_cache(maxsize=None)
def _raw_hits(seed_len, step):
    full, nodes = ref_index(seed_len, step), ref_graph()
    return [ref.raw_hits(full, nodes, r2, seed_len) for r2 in ref_reads()]


def ref_raw_hits(seed_len, step):
    """per read the restatement's raw hits (computed once; no test changes them)"""
    tripwire()
    return _raw_hits(seed_len, step)


@functools.lru_cache(maxsize=None)
def ref_seeds(seed_len, step):
    """per read ref.seed_map (tuples of tuples: immutable)"""
    tripwire()
    full, nodes = ref_index(seed_len, step), ref_graph()
    return [ref.seed_map(full, nodes, r2, seed_len) for r2 in ref_reads()]


@functools.lru_cache(maxsize=None)
def tripwire():
    """The case is still hard, by the restatement alone, at (16, 1) -- a later edit must not quietly make it easy again."""
    seqs, _, reads, n_at = case()
    full = ref_index(16, 1)
    hits = _raw_hits(16, 1)
    flat = [h for per in hits for h in per]
    assert max(len(v) for v in full.values()) >= 100, "no key with >= 100 locations"
    assert any(h[5] > 64 for h in flat), "no right-match run longer than 64 bases (two word borders)"
    assert any(h[4] == 0 and h[0] > 0 for h in flat), "no left extension that stops at the read start"
    assert any((c & 0xFFFFFFFF) + 16 > len(seqs[c >> 32]) for v in full.values() for c in v), "no index entry whose k-mer crosses a node border"
    assert any(h[1] == 0 and h[4] <= n_at < h[4] + h[5] for h in hits[N_SPILL_READ]), "no match run across the N of the N-spill read"
    assert any(len(r) == 0 for r in reads) and any(len(r) == 1 for r in reads)
    return True


def census(seed_len, step):
    """the figures quoted in the test module's docstring"""
    hits = ref_raw_hits(seed_len, step)
    flat = [h for per in hits for h in per]
    full = ref_index(seed_len, step)
    seqs = case()[0]
    return {"hits": len(flat), "max_per_key": max((len(v) for v in full.values()), default=0), "right_gt_64": sum(h[5] > 64 for h in flat),
            "left_at_read_start": sum(h[4] == 0 and h[0] > 0 for h in flat),
            "border_entries": sum((c & 0xFFFFFFFF) + seed_len > len(seqs[c >> 32]) for v in full.values() for c in v)}
