"""Inputs shared by tests/test_pile_alleles_cpu.py and tests/test_pile_alleles_gpu.py: the header's worked values, the packing pinned by
hand, and the batches the device tests add -- the seams of the maximal-run logic, the region's edges, indel calls --, all in
pileup_cases' form (windows [(start, len)], reads, strands, routes)."""
import numpy as np

import pileup_cases as pc
import pyref_pile_alleles as ref
import pyref_pileup

M, I, D = pc.M, pc.I, pc.D
DEL, INS, LONG_INS = ref.DEL, ref.INS, ref.LONG_INS

# ---- the worked values of include/gnx_align.h: window at 100 = ACGTACGTAC -> the events as (pos, kind, key) ----
WORKED = [
    ("ACGAACTAC", [(6, M), (1, D), (3, M)], [(106, DEL, 1)]),
    ("ACGTTTACGTAC", [(4, M), (2, I), (6, M)], [(103, INS, 36)]),
    ("TTTACG", [(3, D), (2, I), (4, M), (3, D)], []),
]

# ---- the packing, pinned by hand: (bases, seq) ----
PACK_PINS = [
    ([3, 3], 36),                                 # TT: 4 | 4 << 3
    ([0], 1), ([4], 5), ([0, 4, 3], 1 | 5 << 3 | 4 << 6),
    ([3] * 21, int("100" * 21, 2)),               # 21 bases fill 63 bits: bit 62 is set, bit 63 is the strand's room
    ([0] * 21, int("001" * 21, 2)),
]


def exact_read(window, route, ins_code=1, subs=()):
    """the read of `route` against `window`: a copy on the M columns (alpha positions in `subs` substituted), ins_code on the I columns"""
    read, w = [], 0
    for r, o in route:
        for _ in range(r):
            if o == M:
                b = int(window[w])
                read.append((b + 1) % 4 if w in subs else b)
                w += 1
            elif o == D:
                w += 1
            else:
                read.append(ins_code)
    return np.asarray(read, dtype=np.uint8)


def _filler(n):
    """n runs that end on an M run: 2M 1I 2M 1I .. 2M (n odd)"""
    assert n % 2 == 1
    return [(2, M) if k % 2 == 0 else (1, I) for k in range(n)]


def seam_plans():
    """(name, route): a maximal D or I run written in every way the kernel can meet it -- run 63 is the last of the first block of 64"""
    zeros_d, zeros_i = [(0, I), (0, M), (0, I)], [(0, D), (0, M), (0, D)]
    return [
        ("d_two_pieces", [(20, M), (2, D), (3, D), (20, M)]),
        ("d_three_pieces", [(20, M), (1, D), (2, D), (3, D), (20, M)]),
        ("i_two_pieces", [(20, M), (2, I), (3, I), (20, M)]),
        ("i_three_pieces", [(20, M), (1, I), (2, I), (3, I), (20, M)]),
        ("d_pieces_with_empty_runs_between", [(20, M), (2, D)] + zeros_d + [(3, D), (0, M), (1, D), (20, M)]),
        ("i_pieces_with_empty_runs_between", [(20, M), (2, I)] + zeros_i + [(3, I), (0, M), (1, I), (20, M)]),
        ("d_over_the_block_seam", _filler(63) + [(2, D), (3, D), (20, M)]),
        ("i_over_the_block_seam", _filler(63) + [(2, I), (3, I), (20, M)]),
        ("d_130_pieces_over_two_seams", [(20, M)] + [(1, D)] * 130 + [(20, M)]),
        ("i_130_pieces_over_two_seams", [(20, M)] + [(1, I)] * 130 + [(20, M)]),
        ("i_20_pieces_over_a_seam", _filler(55) + [(1, I)] * 20 + [(20, M)]),
        ("d_then_a_block_that_begins_empty", _filler(63) + [(2, D)] + zeros_d * 3 + [(3, D), (20, M)]),
        ("i_then_a_block_that_begins_empty", _filler(63) + [(2, I)] + zeros_i * 3 + [(3, I), (20, M)]),
        ("d_closed_by_the_first_run_behind_an_empty_block_start", _filler(63) + [(2, D)] + zeros_d * 2 + [(20, M)]),
        ("d_pieces_with_90_empty_runs_over_a_seam", [(20, M), (2, D)] + zeros_d * 30 + [(4, D), (20, M)]),
        ("i_of_21", [(20, M), (21, I), (20, M)]),
        ("i_of_22", [(20, M), (22, I), (20, M)]),
        ("i_with_an_n", [(20, M), (3, I), (20, M)]),
        ("i_at_alpha_start", [(3, D), (2, I), (20, M)]),
        ("i_first", [(2, I), (20, M)]),
        ("i_at_alpha_end", [(20, M), (2, I), (3, D)]),
        ("i_last", [(20, M), (2, I)]),
        ("leading_and_trailing_d", [(3, D), (20, M), (4, D)]),
        ("one_d_run", [(7, D)]),
        ("one_d_run_in_pieces", [(3, D), (0, M), (4, D)]),
        ("d_then_i_then_d", [(20, M), (2, D), (3, I), (1, D), (20, M)]),
        ("d_of_1_at_a_shared_start", [(20, M), (1, D), (20, M)]),
        ("d_of_7_at_a_shared_start", [(20, M), (7, D), (20, M)]),
    ]


SHARED_START = 7000


def seam_batch(genome):
    """every plan once per strand at the SAME window, with the same read: every allele is seen from both strands.  Windows 211 apart from
    100; the two *_at_a_shared_start plans at SHARED_START: two different deletions at one position."""
    rng = np.random.default_rng(411)
    names, windows, reads, strands, routes = [], [], [], [], []
    at = 100
    for name, route in seam_plans():
        n = sum(r for r, o in route if o != I) + 2  # (two spare bases on either side, as pileup_cases.seam_batch has them)
        start = SHARED_START if name.endswith("_at_a_shared_start") else at
        read = np.concatenate([pc._read_for(rng, genome[start:start + n], route), rng.integers(0, 4, size=2).astype(np.uint8)])
        if name == "i_with_an_n":
            read[21] = 4
        for strand in (0, 1):
            names.append("%s/%d" % (name, strand))
            windows.append((start, n))
            reads.append(read)
            strands.append(strand)
            routes.append(list(route))
        at += 211
    assert at < SHARED_START
    return names, windows, reads, strands, routes


def edge_batch(genome):
    """deletions of 5 that start at lo - 1, lo, hi - 1, hi and insertions of 3 behind the same four positions (pileup_cases.EDGE_REGION =
    [lo, hi)), strands alternating"""
    rng = np.random.default_rng(412)
    lo, hi = pc.EDGE_REGION[0], pc.EDGE_REGION[0] + pc.EDGE_REGION[1]
    windows, reads, strands, routes = [], [], [], []
    for k, x in enumerate((lo - 1, lo, hi - 1, hi)):
        for route, start in (([(20, M), (5, D), (30, M)], x - 20), ([(21, M), (3, I), (30, M)], x - 20)):
            n = sum(r for r, o in route if o != I)
            windows.append((start, n))
            reads.append(pc._read_for(rng, genome[start:start + n], route))
            strands.append(k % 2)
            routes.append(route)
    return windows, reads, strands, routes


def call_batch(genome):
    """pileup_cases.call_batch (a deletion of 2 at 250 and an insertion of CCC behind 281, each with 8 of 12 reads: CALL_OPTS' 2/3 met with
    equality) and on top of it:
      window (1000, 100)  50M 4D 46M, 4 + 3 copies, and 4 plain ones: 7 of 11 at 1050, one read short of 2/3
      window (1500, 100)  50M 1D 49M 2 + 2 copies and 50M 3D 47M 2 + 2 copies: two alleles at 1550, each with 4 of 8
      window (2000, 100)  50M 2I 50M, 5 forward copies: passes, but not with both_strands
      window (30, 100)    35M 2D 63M and 37M 2I 63M, 3 + 3 copies each: alleles at 65 and 66 inside the N run 60 .. 70, silent"""
    windows, reads, strands, routes = (list(x) for x in pc.call_batch(genome))

    def put(start, route, fwd, rev):
        n = sum(r for r, o in route if o != I)
        rd = exact_read(genome[start:start + n], route)
        for k in range(fwd + rev):
            windows.append((start, n))
            reads.append(rd)
            strands.append(0 if k < fwd else 1)
            routes.append(list(route))

    put(1000, [(50, M), (4, D), (46, M)], 4, 3)
    put(1000, [(100, M)], 2, 2)
    put(1500, [(50, M), (1, D), (49, M)], 2, 2)
    put(1500, [(50, M), (3, D), (47, M)], 2, 2)
    put(2000, [(50, M), (2, I), (50, M)], 5, 0)
    put(30, [(35, M), (2, D), (63, M)], 3, 3)
    put(30, [(37, M), (2, I), (63, M)], 3, 3)
    return windows, reads, strands, routes


def restate(genome, region, windows, reads, strands, routes):
    """-> (pyref_pileup's pile, the dict of alleles)"""
    pile = pyref_pileup.new_pile(region[1])
    alleles = ref.new_alleles()
    for (start, n), read, strand, route in zip(windows, reads, strands, routes):
        pyref_pileup.add(pile, pc.LOCAL, start, genome[start:start + n], read, strand, route, region)
        ref.add(alleles, start, read, strand, route, region)
    return pile, alleles


def parse_vcf(text):
    """the records of vcf.WriteVcf's text as (CHROM, POS, REF, ALT, {INFO})"""
    out = []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        assert len(f) == 8 and f[2] == "." and f[5] == "." and f[6] == ".", line
        out.append((f[0], int(f[1]), f[3], f[4], {kv.split("=")[0]: int(kv.split("=")[1]) for kv in f[7].split(";")}))
    return out
