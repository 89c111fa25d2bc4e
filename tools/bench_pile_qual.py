#!/usr/bin/env python
"""Base qualities in the pile and the genotype query on the device: what the quality add costs beside the plain add, and
what gnx_pileup_genotypes costs beside gnx_pileup_calls and beside the memory both read.

The workload of DESIGN.md 4.25 as tools/bench_pileup.py builds it: --reads reads of 150 bases on the synthetic resident reference, half
from the reverse strand, candidates by seed votes (max_cand = 4), HumanChimpTwo -600 / -150, GNX_AFFINE_GAP_LOCAL; the winners in the
orientation they were aligned in, the region = the whole reference; qualities (7 j + 3 k) % 41 + 2 for base j of winner k (2 .. 42).
Legs, alternating in one process, every one on a FRESH pile opened (and switched to quality tracking) outside the timed call, medians of
--rounds rounds after --warmup warm-ups, wall, device (gnx_timing.fill_ms) and kernel-alone (dominant_ms) time:
  add_plain    gnx_pileup_add_by_offset on a plain pile: pile_add_kernel, the comparator
  add_qual_0   gnx_pileup_add_by_offset_qual at min_baseq 0: qual_add_kernel, up to two atomic adds per M column
  add_qual_20  the same at min_baseq 20
Then, on a region of --calls-small and one of --calls-large positions that hold the reads, alternating on ONE quality pile:
  calls        gnx_pileup_calls (reads 14 planes a pass)        genotypes    gnx_pileup_genotypes (reads 12 planes a pass)
Recorded: the ratios of the quality add to the plain add measured in the same process, the atomic adds per second (counted from the
tables themselves: the counters' sum plus the non-zero quality adds), the plane bytes the queries read per second against the 8 TB/s
roofline.  The tables of --check winners are compared with the restatement (tests/pyref_pile_qual.py).  Prints one JSON line and writes
it to --out (default profiles/pile_qual.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_map_reads  # noqa: E402
import bench_summary  # noqa: E402
import pyref_pile_qual  # noqa: E402
from gonomics_amd import _lib, align  # noqa: E402

READ = bench_map_reads.READ
HBM_BYTES_PER_S = 8e12
HOT_AT, HOT_SPAN = 1000000, 1000


def alternate_fresh(legs, rounds, warmup):
    """legs: {name: (setup, fn -> (device ms, kernel ms))}; setup runs outside the timed call.  Medians per leg."""
    wall, dev, ker = ({k: [] for k in legs} for _ in range(3))
    for r in range(warmup + rounds):
        for name, (setup, fn) in legs.items():
            setup()
            t0 = time.perf_counter()
            d, k = fn()
            w = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                wall[name].append(w)
                dev[name].append(d)
                ker[name].append(k)
    return {name: {"wall_ms": statistics.median(wall[name]), "wall_min_ms": min(wall[name]), "wall_max_ms": max(wall[name]), "device_ms": statistics.median(dev[name]),
                   "device_min_ms": min(dev[name]), "device_max_ms": max(dev[name]), "kernel_ms": statistics.median(ker[name])} for name in legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=300, help="winners whose tables are compared with the restatement")
    ap.add_argument("--calls-small", type=int, default=1000000)
    ap.add_argument("--calls-large", type=int, default=64000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pile_qual.json"))
    args = ap.parse_args()
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    _lib.check(L.gnx_init(0, 0))
    _lib.check(L.gnx_set_reference_synthetic(args.ref_len, args.seed))
    reads, _, _ = bench_map_reads.workload(args.reads, args.ref_len, args.seed)
    n = args.reads
    r_cat, r_off = reads.reshape(-1), np.arange(n + 1, dtype=np.int64) * READ
    _lib.reference_index_build(16, 1)
    c_off, c_start, c_len, c_strand, _ = _lib.seed_candidates(r_cat, r_off, **dict(align.SEED_VOTE_DEFAULTS, max_cand=4))
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
    best, _, _, _, ops, off = _lib.best_of_by_offset(p, r_cat, r_off, c_off, c_start, c_len, c_strand)
    placed = np.flatnonzero(best >= 0)
    at = c_off[:-1][placed] + best[placed]
    oriented = reads[placed].copy()  # the winners in the orientation they were aligned in
    strand = c_strand[at].astype(np.uint8)
    rev = strand == 1
    rc = oriented[rev][:, ::-1].copy()
    m = rc < 4
    rc[m] = 3 - rc[m]
    oriented[rev] = rc
    nw = int(placed.shape[0])
    w_cat, w_off = oriented.reshape(-1), np.arange(nw + 1, dtype=np.int64) * READ
    w_ops = np.concatenate([ops[off[r]:off[r + 1]] for r in placed]) if nw else ops[:0]
    w_opsoff = np.concatenate([[0], np.cumsum(np.diff(off)[placed])]).astype(np.int64)
    win_start, win_len = c_start[at].astype(np.int64), c_len[at].astype(np.int64)
    quals = ((7 * np.arange(READ, dtype=np.int64)[None, :] + 3 * np.arange(nw, dtype=np.int64)[:, None]) % 41 + 2).astype(np.uint8)
    q_cat = quals.reshape(-1)

    def fresh(min_baseq, length=None):
        def setup():
            _lib.pileup_open(0, args.ref_len if length is None else length)
            if min_baseq is not None:
                _lib.pileup_track_qualities(min_baseq)
        return setup

    def add_plain(use=None):
        _lib.pileup_add_by_offset(p, w_cat, w_off, win_start, win_len, strand, w_ops, w_opsoff, use=use)
        t = _lib.get_timing()
        return t["fill_ms"], t["dominant_ms"]

    def add_qual(use=None):
        _lib.pileup_add_by_offset_qual(p, w_cat, w_off, win_start, win_len, strand, w_ops, w_opsoff, q_cat, use=use)
        t = _lib.get_timing()
        return t["fill_ms"], t["dominant_ms"]

    res = {"command": "tools/bench_pile_qual.py " + " ".join(sys.argv[1:]), "rounds": args.rounds, "warmup": args.warmup,
           "reads_workload": "%d reads x %d bases on the synthetic reference (%d bases), max_cand 4, HumanChimpTwo -600 / -150, AffineGapLocal; qualities 2 .. 42" % (args.reads, READ, args.ref_len),
           "device_ms_is": "gnx_timing.fill_ms: the base check plus the add kernel; kernel_ms is gnx_timing.dominant_ms: pile_add_kernel / qual_add_kernel alone",
           "winners": nw, "cigar_runs": int(w_ops.shape[0])}
    res.update(alternate_fresh({"add_plain": (fresh(None), add_plain), "add_qual_0": (fresh(0), add_qual), "add_qual_20": (fresh(20), add_qual)}, args.rounds, args.warmup))
    tm = _lib.get_timing()
    res["gnx_timing_last_add"] = {k: tm[k] for k in bench_summary.TIMING_KEYS}
    res["columns"] = int(tm["cells"])
    # the adds of one call, counted from the tables: one call into a fresh pile over one 1 kb stretch every window is moved into (no add reads
    # the reference) -- the counters' sum, and one more add per counted A C G T base, since every quality of the workload is above 0
    hot_start = HOT_AT + win_start % HOT_SPAN
    region = (HOT_AT, HOT_SPAN + int(win_len.max()))
    for name, min_baseq in (("add_plain", None), ("add_qual_0", 0), ("add_qual_20", 20)):
        _lib.pileup_open(*region)
        if min_baseq is None:
            _lib.pileup_add_by_offset(p, w_cat, w_off, hot_start, win_len, strand, w_ops, w_opsoff)
        else:
            _lib.pileup_track_qualities(min_baseq)
            _lib.pileup_add_by_offset_qual(p, w_cat, w_off, hot_start, win_len, strand, w_ops, w_opsoff, q_cat)
        rows = _lib.pileup_get()
        adds = int(rows["base"].sum()) + int(rows["del"].sum()) + int(rows["ins"].sum())
        if min_baseq is not None:
            adds += int(rows["base"][:, :, :4].sum())
        leg = res[name]
        leg["atomic_adds_per_call"] = adds
        leg["atomic_adds_per_s_device"] = adds / max(leg["device_ms"] * 1e-3, 1e-12)
        leg["atomic_adds_per_s_kernel"] = adds / max(leg["kernel_ms"] * 1e-3, 1e-12)
        if name != "add_plain":
            for k in ("wall_ms", "device_ms", "kernel_ms"):
                leg["over_plain_" + k[:-3]] = leg[k] / max(res["add_plain"][k], 1e-9)
    res["qual_pile_device_bytes"] = 72 * args.ref_len  # (14 + 4 planes of int32 over the whole reference)
    # the restatement on the first --check winners, alone in a fresh quality pile over one 1 kb stretch every window is moved into (no add
    # reads the reference: the position, the read byte, the quality and the strand decide it)
    k = min(args.check, nw)
    use = np.zeros(nw, np.uint8)
    use[:k] = 1
    _lib.pileup_open(*region)
    _lib.pileup_track_qualities(20)
    _lib.pileup_add_by_offset_qual(p, w_cat, w_off, hot_start, win_len, strand, w_ops, w_opsoff, q_cat, use=use)
    pile = pyref_pile_qual.new_pile(region[1])
    for q in range(k):
        route = [(int(r), int(o)) for r, o in zip(w_ops["run_length"][w_opsoff[q]:w_opsoff[q + 1]], w_ops["op"][w_opsoff[q]:w_opsoff[q + 1]])]
        pyref_pile_qual.add(pile, 3, int(hot_start[q]), oriented[q], quals[q], int(strand[q]), route, region, 20)
    got, got_q = _lib.pileup_get(), _lib.pileup_get_qual()
    want, want_q = pyref_pile_qual.rows(pile)
    res["checked_against_restatement"] = k
    res["restatement_agrees"] = bool(all([g["base"][0].tolist(), g["base"][1].tolist(), g["del"].tolist(), g["ins"].tolist()] == w for g, w in zip(got, want)) and got_q.tolist() == want_q)
    # the two queries on one quality pile that holds the reads
    for name, length in (("small", min(args.calls_small, args.ref_len)), ("large", min(args.calls_large, args.ref_len))):
        fresh(0, length)()
        add_qual()
        counts = {"calls": 0, "genotypes": 0}

        def calls():
            counts["calls"] = int(_lib.pileup_calls(1, 1, 1, 2, 0).shape[0])
            t = _lib.get_timing()
            return t["fill_ms"], t["dominant_ms"]

        def genotypes():
            counts["genotypes"] = int(_lib.pileup_genotypes(1).shape[0])
            t = _lib.get_timing()
            return t["fill_ms"], t["dominant_ms"]
        legs = alternate_fresh({"calls": (lambda: None, calls), "genotypes": (lambda: None, genotypes)}, args.rounds, args.warmup)
        for leg_name, planes in (("calls", 14), ("genotypes", 12)):
            leg = legs[leg_name]
            passes = 2 if counts[leg_name] else 1
            plane_bytes = planes * 4 * int(length)
            leg.update({"positions": int(length), "records": counts[leg_name], "planes": planes, "plane_bytes": plane_bytes, "passes": passes,
                        "plane_bytes_read_per_s": plane_bytes * passes / max(leg["device_ms"] * 1e-3, 1e-12)})
            leg["share_of_8TBps_roofline"] = leg["plane_bytes_read_per_s"] / HBM_BYTES_PER_S
            res["%s_%s" % (leg_name, name)] = leg
        res["genotypes_over_calls_device_" + name] = legs["genotypes"]["device_ms"] / max(legs["calls"]["device_ms"], 1e-9)
    _lib.pileup_close()
    _lib.check(L.gnx_set_reference(None, 0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
