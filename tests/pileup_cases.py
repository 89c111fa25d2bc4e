"""Inputs shared by tests/test_pileup_cpu.py and tests/test_pileup_gpu.py: the header's worked values, the call rule pinned by hand, and
the batches the device tests add (the summary's seam cases re-based as windows of one reference, region edges, contention, calls)."""
import numpy as np

import pyref_pileup as ref
import summary_cases as sc
import test_summary_gpu as tsg

M, I, D = sc.M, sc.I, sc.D
LOCAL = sc.LOCAL
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}

# ---- the worked values of include/gnx_align.h: window at 100 = ACGTACGTAC ----
ALPHA, ALPHA_AT = "ACGTACGTAC", 100
# (read, route, what lies where: position -> a base letter or "del")
WORKED = [
    ("ACGAACTAC", [(6, M), (1, D), (3, M)], {100: "A", 101: "C", 102: "G", 103: "A", 104: "A", 105: "C", 106: "del", 107: "T", 108: "A", 109: "C"}),
    ("TTTACG", [(3, D), (2, I), (4, M), (3, D)], {103: "T", 104: "A", 105: "C", 106: "G"}),
]


def worked_pile(where, strand, region):
    """the pile a worked value must give, written down from its table (not computed)"""
    pile = ref.new_pile(region[1])
    for pos, what in where.items():
        if region[0] <= pos < region[0] + region[1]:
            row = pile[pos - region[0]]
            if what == "del":
                row["del"][strand] += 1
            else:
                row["base"][strand][CODE[what]] += 1
    return pile


# ---- the call rule, pinned by hand ----
def row(fwd=(0, 0, 0, 0, 0), rev=(0, 0, 0, 0, 0), dele=(0, 0), ins=(0, 0)):
    return {"base": [list(fwd), list(rev)], "del": list(dele), "ins": list(ins)}


def opts(min_depth=1, min_alt=1, frac=(1, 2), both_strands=0):
    return {"min_depth": min_depth, "min_alt": min_alt, "frac_num": frac[0], "frac_den": frac[1], "both_strands": both_strands}


SUB, DEL, INS = ref.SUB, ref.DEL, ref.INS
# (name, reference code, row, options, the calls at that position as (depth, count, count_fwd, kind, ref, alt))
CALL_PINS = [
    ("substitution", 0, row(fwd=(2, 0, 6, 0, 0), rev=(0, 0, 2, 0, 0)), opts(), [(10, 8, 6, SUB, 0, 2)]),
    ("deletion", 1, row(fwd=(0, 3, 0, 0, 0), dele=(4, 3)), opts(), [(10, 7, 4, DEL, 1, 0xFF)]),
    ("insertion", 2, row(fwd=(0, 0, 5, 0, 0), rev=(0, 0, 5, 0, 0), ins=(3, 3)), opts(), [(10, 6, 3, INS, 2, 0xFF)]),
    ("primary_then_insertion", 2, row(fwd=(0, 0, 1, 5, 0), rev=(0, 0, 1, 3, 0), ins=(2, 4)), opts(), [(10, 8, 5, SUB, 2, 3), (10, 6, 2, INS, 2, 0xFF)]),
    ("tie_of_two_bases", 3, row(fwd=(4, 1, 0, 2, 0), rev=(0, 3, 0, 0, 0)), opts(frac=(1, 3)), [(10, 4, 4, SUB, 3, 0)]),
    ("tie_of_base_and_deletion", 0, row(fwd=(1, 0, 2, 0, 0), rev=(0, 0, 2, 0, 0), dele=(4, 0)), opts(frac=(1, 3)), [(9, 4, 2, SUB, 0, 2)]),
    ("deletion_beats_a_smaller_base", 0, row(fwd=(1, 0, 2, 0, 0), rev=(0, 0, 1, 0, 0), dele=(4, 0)), opts(frac=(1, 3)), [(8, 4, 4, DEL, 0, 0xFF)]),
    ("fraction_met_with_equality", 0, row(fwd=(3, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(), [(10, 5, 5, SUB, 0, 1)]),
    ("one_read_fewer_fails", 0, row(fwd=(3, 4, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(), []),
    ("min_alt_met_with_equality", 0, row(fwd=(3, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(min_alt=5), [(10, 5, 5, SUB, 0, 1)]),
    ("min_alt_missed", 0, row(fwd=(3, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(min_alt=6), []),
    ("min_depth_met_with_equality", 0, row(fwd=(3, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(min_depth=10), [(10, 5, 5, SUB, 0, 1)]),
    ("min_depth_missed", 0, row(fwd=(3, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(min_depth=11), []),
    ("both_strands_off", 0, row(fwd=(0, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(), [(7, 5, 5, SUB, 0, 1)]),
    ("both_strands_on_one_strand_only", 0, row(fwd=(0, 5, 0, 0, 0), rev=(2, 0, 0, 0, 0)), opts(both_strands=1), []),
    ("both_strands_on_reverse_only", 0, row(fwd=(2, 0, 0, 0, 0), rev=(0, 5, 0, 0, 0)), opts(both_strands=1), []),
    ("both_strands_on_both", 0, row(fwd=(0, 4, 0, 0, 0), rev=(2, 1, 0, 0, 0)), opts(both_strands=1), [(7, 5, 4, SUB, 0, 1)]),
    ("both_strands_insertion", 0, row(fwd=(4, 0, 0, 0, 0), ins=(4, 0)), opts(both_strands=1), []),
    ("reference_n_is_silent", 4, row(fwd=(0, 9, 0, 0, 0), rev=(0, 9, 0, 0, 0), dele=(3, 3), ins=(9, 9)), opts(), []),
    ("read_n_is_depth_not_a_candidate", 0, row(fwd=(0, 3, 0, 0, 7), rev=(0, 0, 0, 0, 0)), opts(frac=(1, 4)), [(10, 3, 3, SUB, 0, 1)]),
    ("the_reference_base_is_no_candidate", 1, row(fwd=(0, 9, 0, 0, 0), rev=(0, 0, 1, 0, 0)), opts(frac=(1, 10)), [(10, 1, 0, SUB, 1, 2)]),
    ("nothing_there", 0, row(), opts(), []),
]


# ---- batches for the device: (windows [(start, len)], reads, strands, routes) ----
def _read_for(rng, window, route):
    """the read of `route` against `window` (alpha): a copy on the M columns with a tenth of them substituted, N among the substitutes"""
    return tsg._read_for(rng, window, route, True)


def seam_batch(genome):
    """the summary's seam cases as windows of `genome`, every case once per strand: window k starts where a stride of 389 puts it --
    every dword phase, some over the N runs of the genome --, is as long as the alpha bases its route consumes plus two spare ones"""
    rng = np.random.default_rng(311)
    names, windows, reads, strands, routes = [], [], [], [], []
    at = 0
    for name, _, _, route in sc.seam_cases():
        n = sum(r for r, o in route if o != I) + 2
        for strand in (0, 1):
            if at + n > len(genome):
                at = 7
            names.append("%s/%d" % (name, strand))
            windows.append((at, n))
            reads.append(np.concatenate([_read_for(rng, genome[at:at + n], route), rng.integers(0, 4, size=2).astype(np.uint8)]))
            strands.append(strand)
            routes.append(list(route))
            at += 389
    return names, windows, reads, strands, routes


EDGE_REGION = (40, 4160)  # [40, 4200)


def edge_batch(genome):
    """reads around the edges of EDGE_REGION: starting before 40, ending after 4200, wholly outside on either side, a D run crossing
    either edge, an I run behind position 39 (dropped) and one behind 4199 (kept)"""
    rng = np.random.default_rng(312)
    lo, hi = EDGE_REGION[0], EDGE_REGION[0] + EDGE_REGION[1]
    plans = [
        (lo - 30, [(100, M)]),                                   # starts before the region
        (hi - 50, [(100, M)]),                                   # ends behind it
        (0, [(30, M)]), (lo - 1, [(1, M)]), (hi, [(90, M)]), (hi + 500, [(40, M), (2, D), (40, M)]),  # wholly outside
        (lo - 20, [(17, M), (6, D), (60, M)]),                   # a D run over the left edge: alpha 17 .. 22 = positions 37 .. 42
        (hi - 50, [(47, M), (6, D), (30, M)]),                   # a D run over the right edge: positions 4197 .. 4202
        (lo - 20, [(20, M), (3, I), (50, M)]),                   # an I run behind position 39: dropped
        (lo - 20, [(21, M), (3, I), (50, M)]),                   # ... behind position 40: kept
        (hi - 60, [(60, M), (2, I), (30, M)]),                   # an I run behind position 4199: kept
        (hi - 60, [(61, M), (2, I), (30, M)]),                   # ... behind position 4200: dropped
        (lo, [(5, D), (80, M), (4, D)]), (hi - 80, [(3, D), (70, M), (7, D)]),  # free end gaps at the edges
    ]
    windows, reads, strands, routes = [], [], [], []
    for k, (start, route) in enumerate(plans):
        n = sum(r for r, o in route if o != I)
        windows.append((start, n))
        reads.append(_read_for(rng, genome[start:start + n], route))
        strands.append(k % 2)
        routes.append(route)
    return windows, reads, strands, routes


CONTENTION_ROUTE = [(50, M), (1, D), (40, M), (2, I), (58, M)]  # a 150-base read with a deletion and an insertion; the substitution: alpha 20


def contention_batch(genome, copies=256, start=1000):
    n = sum(r for r, o in CONTENTION_ROUTE if o != I)
    window = genome[start:start + n]
    read = []
    w = 0
    for r, o in CONTENTION_ROUTE:
        for _ in range(r):
            if o == M:
                read.append(int(window[w]))
                w += 1
            elif o == D:
                w += 1
            else:
                read.append(2)
    read = np.asarray(read, dtype=np.uint8)
    assert read.shape[0] == 150
    read[20] = (read[20] + 1) % 4
    return [(start, n)] * copies, [read] * copies, [0] * copies, [list(CONTENTION_ROUTE)] * copies


CALL_REGION = (0, 4200)
CALL_OPTS = opts(min_depth=1, min_alt=2, frac=(2, 3))


def call_batch(genome):
    """piles that hold every kind of call in region [0, 4200) of test_summary_gpu._resident_cases()'s genome (N at 60 .. 70 and 4090 .. 4100):
      window (30, 100), 100M, 6 forward + 4 reverse copies: a substitution at 70 (all reads), one at 65 inside the first N run (silent)
      window (200, 120), 50M 2D 30M 3I 38M, 5 + 3 copies with a substitution at alpha 81, and 4 copies of the window itself:
        a deletion at 250 / 251 with 8 of 12, an insertion behind 281 with 8 of 12 and a substitution AT 281 with 8 of 12 -- 2/3 each, met
        with equality
      window (4050, 100), 100M, 3 copies with a substitution at 4095 inside the second N run (silent) and one at 4060"""
    def copy_of(window, route, subs):
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
                    read.append(1)
        return np.asarray(read, dtype=np.uint8)

    windows, reads, strands, routes = [], [], [], []

    def put(start, route, subs, fwd, rev):
        n = sum(r for r, o in route if o != I)
        rd = copy_of(genome[start:start + n], route, subs)
        for k in range(fwd + rev):
            windows.append((start, n))
            reads.append(rd)
            strands.append(0 if k < fwd else 1)
            routes.append(list(route))

    put(30, [(100, M)], {40, 35}, 6, 4)
    put(200, [(50, M), (2, D), (30, M), (3, I), (38, M)], {81}, 5, 3)
    put(200, [(120, M)], set(), 2, 2)
    put(4050, [(100, M)], {45, 10}, 2, 1)
    return windows, reads, strands, routes


def restate(genome, region, windows, reads, strands, routes):
    pile = ref.new_pile(region[1])
    for (start, n), read, strand, route in zip(windows, reads, strands, routes):
        ref.add(pile, LOCAL, start, genome[start:start + n], read, strand, route, region)
    return pile
