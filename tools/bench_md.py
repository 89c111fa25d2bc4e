#!/usr/bin/env python
"""MD strings on the device (gnx_md_*): what they cost beside the summary call they follow.

The workload of DESIGN.md 4.18: --reads reads of 150 bases on the synthetic resident reference, half from the reverse strand,
candidates by seed votes (max_cand = 4), HumanChimpTwo -600 / -150, GNX_AFFINE_GAP_LOCAL.  Legs, alternating in one process:
gnx_md_batch_by_offset on the winners, and the unchanged gnx_summarize_batch_by_offset with the extended CIGAR on the same winners
(the comparator: the same two walks over the same columns).  Every figure is the median of --rounds rounds after --warmup warm-ups,
tools/bench_summary.py's method.  The strings of the timed call are checked: the three invariants of include/gnx_align.h against the
summary of the same call, and byte equality with the restatement (tests/pyref_md.py) on --check reads against the host's copy of
their windows.  Prints one JSON line and writes it to --out (default profiles/aln_md.json)."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_map_reads  # noqa: E402
import bench_summary  # noqa: E402
import pyref_md  # noqa: E402
from gonomics_amd import _lib, align  # noqa: E402

READ = bench_map_reads.READ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=500, help="winners whose string is compared with the restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aln_md.json"))
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
    rev = c_strand[at] == 1
    rc = oriented[rev][:, ::-1].copy()
    m = rc < 4
    rc[m] = 3 - rc[m]
    oriented[rev] = rc
    w_cat, w_off = oriented.reshape(-1), np.arange(placed.shape[0] + 1, dtype=np.int64) * READ
    w_ops = np.concatenate([ops[off[r]:off[r + 1]] for r in placed]) if placed.shape[0] else ops[:0]
    w_opsoff = np.concatenate([[0], np.cumsum(np.diff(off)[placed])]).astype(np.int64)
    win_start, win_len = c_start[at], c_len[at]

    def md():
        _lib.md_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff)
        return _lib.get_timing()["fill_ms"]

    def summary():
        _lib.summarize_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff, xcigar=True)
        return _lib.get_timing()["fill_ms"]
    res = {"command": "tools/bench_md.py " + " ".join(sys.argv[1:]), "rounds": args.rounds, "warmup": args.warmup,
           "reads_workload": "%d reads x %d bases on the synthetic reference (%d bases), max_cand 4, HumanChimpTwo -600 / -150, AffineGapLocal" % (args.reads, READ, args.ref_len)}
    res.update(bench_summary.alternate({"md_winners": md, "summarize_winners_xcigar": summary}, args.rounds, args.warmup))
    res["md_over_summary_device"] = res["md_winners"]["device_ms"] / max(res["summarize_winners_xcigar"]["device_ms"], 1e-9)
    res["md_over_summary_wall"] = res["md_winners"]["wall_ms"] / max(res["summarize_winners_xcigar"]["wall_ms"], 1e-9)
    text, t_off = _lib.md_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff)
    tm = _lib.get_timing()
    out, _, _ = _lib.summarize_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff)
    strings = _lib.md_strings(text, t_off)
    numbers = letters = deleted = 0
    for s in strings:
        a, b, c = pyref_md.parts(s)
        numbers, letters, deleted = numbers + a, letters + b, deleted + c
    events = sum(len(re.findall(r"[A-Z]", s)) for s in strings)
    res.update({"winners": int(placed.shape[0]), "cigar_runs": int(w_ops.shape[0]), "columns": int(tm["cells"]), "md_bytes": int(text.shape[0]), "events": int(events),
                "events_per_column": events / max(int(tm["cells"]), 1),
                "gnx_timing_last_call": {k: tm[k] for k in bench_summary.TIMING_KEYS},
                "invariants_hold": bool((numbers, letters, deleted) == (int(out["n_equal"].sum()), int(out["n_mismatch"].sum()), int(out["del_bases"].sum())))})
    same = True
    for k in range(min(args.check, placed.shape[0])):
        route = [(int(r), int(o)) for r, o in zip(w_ops["run_length"][w_opsoff[k]:w_opsoff[k + 1]], w_ops["op"][w_opsoff[k]:w_opsoff[k + 1]])]
        target = _lib.synthetic_reference_bases(int(win_start[k]), int(win_len[k]), args.seed)
        same = same and strings[k] == pyref_md.md(3, target, oriented[k], route)
    res["checked_against_restatement"] = min(args.check, int(placed.shape[0]))
    res["restatement_agrees"] = bool(same)
    _lib.check(L.gnx_set_reference(None, 0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
