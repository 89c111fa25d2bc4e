#!/usr/bin/env python
"""The alleles of the pile (gnx_pileup_track_alleles .. gnx_pileup_indel_calls): what tracking costs an add, and what
the two queries cost.

The workload of DESIGN.md 4.25 as tools/bench_pileup.py builds it: --reads reads of 150 bases on the synthetic resident reference, half
from the reverse strand, candidates by seed votes (max_cand = 4), HumanChimpTwo -600 / -150, GNX_AFFINE_GAP_LOCAL; the winners in the
orientation they were aligned in, the region = the whole reference.  Legs, alternating in one process, medians of --rounds rounds
after --warmup warm-ups, wall and device time (gnx_timing.fill_ms); every round opens a fresh pile for (a) and one for (b), so (c)
and (d) see the events of exactly one add:
  (a) add            gnx_pileup_add_by_offset on a pile that does not track; add_again: the same call once more on the same pile
  (b) add_tracking   the same call on a tracking pile (allele_log_kernel behind pile_add_kernel)
  (c) alleles        gnx_pileup_alleles: two radix sorts of the log, the reduce
  (d) indel_calls    gnx_pileup_indel_calls (min_depth 1, min_alt 1, 1/2): the same and the call kernels
Before them add_alone: rounds of open + add and nothing else, which is all a library without the allele entries (the parent commit's,
loaded through GNX_LIB_PATH) can run: the same kernel in the same sequence of calls, for the session's drift.  The alleles of --check
winners are compared with the restatement (tests/pyref_pile_alleles.py).  Prints one JSON line and writes it to --out (default
profiles/pile_alleles.json; "" = nowhere)."""
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
import pyref_pile_alleles  # noqa: E402
from gonomics_amd import _lib, align  # noqa: E402

READ = bench_map_reads.READ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=300, help="winners whose alleles are compared with the restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pile_alleles.json"))
    args = ap.parse_args()
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    tracking = hasattr(L, "gnx_pileup_track_alleles")
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
    w_cat, w_off = oriented.reshape(-1), np.arange(placed.shape[0] + 1, dtype=np.int64) * READ
    w_ops = np.concatenate([ops[off[r]:off[r + 1]] for r in placed]) if placed.shape[0] else ops[:0]
    w_opsoff = np.concatenate([[0], np.cumsum(np.diff(off)[placed])]).astype(np.int64)
    win_start, win_len = c_start[at].astype(np.int64), c_len[at].astype(np.int64)

    def add():
        _lib.pileup_add_by_offset(p, w_cat, w_off, win_start, win_len, strand, w_ops, w_opsoff)

    legs = ["add_alone"] + (["add", "add_again", "add_tracking", "alleles", "indel_calls"] if tracking else [])
    wall, dev, kern = {k: [] for k in legs}, {k: [] for k in legs}, {k: [] for k in legs}
    counts = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        wall[name].append((time.perf_counter() - t0) * 1e3)
        t = _lib.get_timing()
        dev[name].append(t["fill_ms"])
        kern[name].append(t["dominant_ms"])
        return out

    for r in range(args.warmup + args.rounds):
        _lib.pileup_open(0, args.ref_len)
        timed("add_alone", add)
    for r in range(args.warmup + args.rounds if tracking else 0):
        _lib.pileup_open(0, args.ref_len)
        timed("add", add)
        timed("add_again", add)
        _lib.pileup_open(0, args.ref_len)
        _lib.pileup_track_alleles(0)
        timed("add_tracking", add)
        counts["n_events"] = _lib.pileup_allele_info()["events"]
        counts["n_alleles"] = int(timed("alleles", _lib.pileup_alleles).shape[0])
        counts["n_indel_calls"] = int(timed("indel_calls", lambda: _lib.pileup_indel_calls(1, 1, 1, 2, 0)).shape[0])
    res = {"command": "tools/bench_pile_alleles.py " + " ".join(sys.argv[1:]), "library": os.path.basename(_lib.LIB_PATH), "library_tracks_alleles": tracking,
           "rounds": args.rounds, "warmup": args.warmup, "winners": int(placed.shape[0]), "cigar_runs": int(w_ops.shape[0]),
           "reads_workload": "%d reads x %d bases on the synthetic reference (%d bases), max_cand 4, HumanChimpTwo -600 / -150, AffineGapLocal" % (args.reads, READ, args.ref_len),
           "device_ms_is": "gnx_timing.fill_ms; kernel_ms is gnx_timing.dominant_ms (the add legs: pile_add_kernel alone; indel_calls: the call kernels alone)"}
    res.update(counts)
    for name in legs:
        w, d, k = wall[name][args.warmup:], dev[name][args.warmup:], kern[name][args.warmup:]
        res[name] = {"wall_ms": statistics.median(w), "wall_min_ms": min(w), "wall_max_ms": max(w), "device_ms": statistics.median(d), "device_min_ms": min(d),
                     "device_max_ms": max(d), "kernel_ms": statistics.median(k)}
    if tracking:
        res["add_tracking"]["over_add_device"] = res["add_tracking"]["device_ms"] / max(res["add"]["device_ms"], 1e-9)
        res["add_tracking"]["events_per_s_allele_kernel"] = counts["n_events"] / max((res["add_tracking"]["device_ms"] - res["add"]["device_ms"]) * 1e-3, 1e-12)
        res["alleles"]["events_per_s"] = counts["n_events"] / max(res["alleles"]["device_ms"] * 1e-3, 1e-12)
        # the restatement on the first --check winners, alone in a fresh tracking pile
        k = min(args.check, int(placed.shape[0]))
        use = np.zeros(placed.shape[0], np.uint8)
        use[:k] = 1
        _lib.pileup_open(0, args.ref_len)
        _lib.pileup_track_alleles(1)
        _lib.pileup_add_by_offset(p, w_cat, w_off, win_start, win_len, strand, w_ops, w_opsoff, use=use)
        want = pyref_pile_alleles.new_alleles()
        for q in range(k):
            route = [(int(r), int(o)) for r, o in zip(w_ops["run_length"][w_opsoff[q]:w_opsoff[q + 1]], w_ops["op"][w_opsoff[q]:w_opsoff[q + 1]])]
            pyref_pile_alleles.add(want, int(win_start[q]), oriented[q], int(strand[q]), route, (0, args.ref_len))
        got = [(int(a["pos"]), int(a["kind"]), int(a["seq"]) if a["kind"] == 2 else int(a["length"]), int(a["count"]), int(a["count_fwd"])) for a in _lib.pileup_alleles()]
        res["checked_against_restatement"] = k
        res["restatement_agrees"] = bool(got == pyref_pile_alleles.listed(want))
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
