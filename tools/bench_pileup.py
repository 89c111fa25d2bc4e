#!/usr/bin/env python
"""The pile on the device (gnx_pileup_*): what adding finished alignments costs beside the same walk without atomics,
and what turning the pile into calls costs beside the memory it reads.

The workload of DESIGN.md 4.23 (a) as tools/bench_md.py builds it: --reads reads of 150 bases on the synthetic resident reference,
half from the reverse strand, candidates by seed votes (max_cand = 4), HumanChimpTwo -600 / -150, GNX_AFFINE_GAP_LOCAL; the winners in
the orientation they were aligned in.  Legs, alternating in one process, medians of --rounds rounds after --warmup warm-ups
(tools/bench_summary.py's method), wall and device time:
  comparator   gnx_summarize_batch_by_offset without the extended CIGAR, unchanged: the same walk without atomics
  spread       gnx_pileup_add_by_offset, the region = the whole reference, the windows where the reads were placed
  hot          the same call with every window moved into one 1 kb stretch: the contention of a deep amplicon
Then gnx_pileup_calls over a region of --calls-small and one of --calls-large positions that hold the spread reads.
Recorded: the add / comparator ratios, the atomic adds per second both placements imply (the adds of one call are counted from the
table itself), the bytes of planes the calls read per second against the 8 TB/s roofline.  The counts of --check winners are compared
with the restatement (tests/pyref_pileup.py).  Prints one JSON line and writes it to --out (default profiles/pileup.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_map_reads  # noqa: E402
import bench_summary  # noqa: E402
import pyref_pileup  # noqa: E402
from gonomics_amd import _lib, align  # noqa: E402

READ = bench_map_reads.READ
HBM_BYTES_PER_S = 8e12
HOT_AT, HOT_SPAN = 1000000, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=300, help="winners whose counts are compared with the restatement")
    ap.add_argument("--calls-small", type=int, default=1000000)
    ap.add_argument("--calls-large", type=int, default=64000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup.json"))
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
    w_cat, w_off = oriented.reshape(-1), np.arange(placed.shape[0] + 1, dtype=np.int64) * READ
    w_ops = np.concatenate([ops[off[r]:off[r + 1]] for r in placed]) if placed.shape[0] else ops[:0]
    w_opsoff = np.concatenate([[0], np.cumsum(np.diff(off)[placed])]).astype(np.int64)
    win_start, win_len = c_start[at].astype(np.int64), c_len[at].astype(np.int64)
    hot_start = HOT_AT + win_start % HOT_SPAN  # every window starts inside one 1 kb stretch
    hot_region = (HOT_AT, HOT_SPAN + int(win_len.max()))

    def comparator():
        _lib.summarize_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff)
        return _lib.get_timing()["fill_ms"]

    kernel_ms = {"spread": [], "hot": []}

    def add(name, starts):
        def leg():
            _lib.pileup_add_by_offset(p, w_cat, w_off, starts, win_len, strand, w_ops, w_opsoff)
            t = _lib.get_timing()
            kernel_ms[name].append(t["dominant_ms"])
            return t["fill_ms"]
        return leg

    res = {"command": "tools/bench_pileup.py " + " ".join(sys.argv[1:]), "rounds": args.rounds, "warmup": args.warmup,
           "reads_workload": "%d reads x %d bases on the synthetic reference (%d bases), max_cand 4, HumanChimpTwo -600 / -150, AffineGapLocal" % (args.reads, READ, args.ref_len),
           "device_ms_is": "gnx_timing.fill_ms: the base check plus the walk (comparator: aln_summary_kernel, add legs: pile_add_kernel); add_kernel_ms is pile_add_kernel alone"}
    _lib.pileup_open(0, args.ref_len)
    res["pile_device_bytes"] = _lib.pileup_info()["device_bytes"]
    res.update(bench_summary.alternate({"comparator_summarize": comparator, "add_spread": add("spread", win_start), "add_hot": add("hot", hot_start)}, args.rounds, args.warmup))
    tm = _lib.get_timing()
    res["gnx_timing_last_add"] = {k: tm[k] for k in bench_summary.TIMING_KEYS}
    # the adds of one call, counted from the table: one call into a fresh pile over the hot stretch, which holds every moved window
    _lib.pileup_open(*hot_region)
    _lib.pileup_add_by_offset(p, w_cat, w_off, hot_start, win_len, strand, w_ops, w_opsoff)
    rows = _lib.pileup_get()
    adds = int(rows["base"].sum()) + int(rows["del"].sum()) + int(rows["ins"].sum())
    out, _, _ = _lib.summarize_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff)
    res.update({"winners": int(placed.shape[0]), "cigar_runs": int(w_ops.shape[0]), "columns": int(tm["cells"]), "atomic_adds_per_call": adds,
                "adds_match_the_summary": bool(int(rows["base"].sum()) == int((out["n_equal"] + out["n_mismatch"]).sum()) and int(rows["del"].sum()) == int(out["del_bases"].sum())
                                               and int(rows["ins"].sum()) <= int(out["gap_runs"].sum())),
                "hot_max_counter": int(max(rows["base"].max(), rows["del"].max(), rows["ins"].max()))})
    for name in ("spread", "hot"):
        leg = res["add_" + name]
        k_ms = float(np.median(kernel_ms[name][args.warmup:]))
        leg["add_kernel_ms"] = k_ms
        leg["over_comparator_device"] = leg["device_ms"] / max(res["comparator_summarize"]["device_ms"], 1e-9)
        leg["over_comparator_wall"] = leg["wall_ms"] / max(res["comparator_summarize"]["wall_ms"], 1e-9)
        leg["atomic_adds_per_s_device"] = adds / max(leg["device_ms"] * 1e-3, 1e-12)
        leg["atomic_adds_per_s_add_kernel"] = adds / max(k_ms * 1e-3, 1e-12)
    # the restatement on the first --check winners, alone in a fresh pile over the hot stretch
    k = min(args.check, int(placed.shape[0]))
    use = np.zeros(placed.shape[0], np.uint8)
    use[:k] = 1
    _lib.pileup_open(*hot_region)
    _lib.pileup_add_by_offset(p, w_cat, w_off, hot_start, win_len, strand, w_ops, w_opsoff, use=use)
    pile = pyref_pileup.new_pile(hot_region[1])
    for q in range(k):
        route = [(int(r), int(o)) for r, o in zip(w_ops["run_length"][w_opsoff[q]:w_opsoff[q + 1]], w_ops["op"][w_opsoff[q]:w_opsoff[q + 1]])]
        pyref_pileup.add(pile, 3, int(hot_start[q]), None, oriented[q], int(strand[q]), route, hot_region)
    got = _lib.pileup_get()
    want = pyref_pileup.rows(pile)
    res["checked_against_restatement"] = k
    res["restatement_agrees"] = bool(all([g["base"][0].tolist(), g["base"][1].tolist(), g["del"].tolist(), g["ins"].tolist()] == w for g, w in zip(got, want)))
    # calls: regions that hold the spread reads
    for name, length in (("calls_small", min(args.calls_small, args.ref_len)), ("calls_large", min(args.calls_large, args.ref_len))):
        _lib.pileup_open(0, length)
        _lib.pileup_add_by_offset(p, w_cat, w_off, win_start, win_len, strand, w_ops, w_opsoff)
        n_calls = [0]

        def calls():
            n_calls[0] = int(_lib.pileup_calls(1, 1, 1, 2, 0).shape[0])
            return _lib.get_timing()["fill_ms"]
        leg = bench_summary.alternate({name: calls}, args.rounds, args.warmup)[name]
        plane_bytes = _lib.pileup_info()["device_bytes"]
        leg.update({"positions": int(length), "calls": n_calls[0], "plane_bytes": plane_bytes, "passes": 2 if n_calls[0] else 1,
                    "plane_bytes_read_per_s": plane_bytes * (2 if n_calls[0] else 1) / max(leg["device_ms"] * 1e-3, 1e-12)})
        leg["share_of_8TBps_roofline"] = leg["plane_bytes_read_per_s"] / HBM_BYTES_PER_S
        res[name] = leg
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
