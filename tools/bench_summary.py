#!/usr/bin/env python
"""Alignment summaries on the device (gnx_summarize_*): what they cost beside the calls they follow.

(a) The workload of DESIGN.md 4.18: --reads reads of 150 bases on the synthetic resident reference, half from the reverse strand,
    candidates by seed votes (max_cand = 4), HumanChimpTwo -600 / -150, GNX_AFFINE_GAP_LOCAL.  Legs, alternating in one process:
    gnx_best_of_by_offset with its CIGAR stage (the unchanged entry: the comparator), the same without it (their difference in device
    time is the CIGAR stage), and gnx_summarize_batch_by_offset on the winners with and without the extended CIGAR.
(b) One long pair each: ConstGap 300 kb x 2 Mb and AffineGap 1 Mb x 1 Mb, generated as tools/long_pairs.py generates them.  Legs: the
    device summary against the host re-score the project's tests use on the same CIGAR (rescore_const / rescore_affine, numpy), and
    that both agree on the score and the consumed lengths.
Every figure is the median of --rounds rounds after --warmup warm-ups.  Prints one JSON line and writes it to --out (default
profiles/aln_summary.json)."""
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
import long_pairs  # noqa: E402
from gonomics_amd import _lib, align  # noqa: E402

READ = bench_map_reads.READ
TIMING_KEYS = ("fast_path", "fill_ms", "dominant_ms", "total_ms", "host_ms", "cells", "n_launches")


def alternate(legs, rounds, warmup):
    """legs: {name: fn -> device ms or None}.  Returns {name: {"wall_ms": median, "device_ms": median, ...}}"""
    wall = {k: [] for k in legs}
    dev = {k: [] for k in legs}
    for r in range(warmup + rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            d = fn()
            w = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                wall[name].append(w)
                dev[name].append(d)
    out = {}
    for name in legs:
        out[name] = {"wall_ms": statistics.median(wall[name]), "wall_min_ms": min(wall[name]), "wall_max_ms": max(wall[name])}
        if dev[name][0] is not None:
            out[name].update({"device_ms": statistics.median(dev[name]), "device_min_ms": min(dev[name]), "device_max_ms": max(dev[name])})
    return out


def reads_leg(args):
    L = _lib.lib()
    _lib.check(L.gnx_set_reference_synthetic(args.ref_len, args.seed))
    reads, origin, strand = bench_map_reads.workload(args.reads, args.ref_len, args.seed)
    n = args.reads
    r_cat, r_off = reads.reshape(-1), np.arange(n + 1, dtype=np.int64) * READ
    _lib.reference_index_build(16, 1)
    opts = dict(align.SEED_VOTE_DEFAULTS, max_cand=4)
    c_off, c_start, c_len, c_strand, _ = _lib.seed_candidates(r_cat, r_off, **opts)
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
    best, scores, ends, _, ops, off = _lib.best_of_by_offset(p, r_cat, r_off, c_off, c_start, c_len, c_strand)
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

    def best_of(cigar):
        _lib.best_of_by_offset(p, r_cat, r_off, c_off, c_start, c_len, c_strand, cigar=cigar)
        return _lib.get_timing()["total_ms"]

    def summary(xcigar):
        _lib.summarize_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff, xcigar=xcigar)
        return _lib.get_timing()["fill_ms"]
    res = alternate({"best_of_with_cigars": lambda: best_of(True), "best_of_scores_only": lambda: best_of(False),
                     "summarize_winners": lambda: summary(False), "summarize_winners_xcigar": lambda: summary(True)}, args.rounds, args.warmup)
    out, _, _ = _lib.summarize_batch_by_offset(p, w_cat, w_off, win_start, win_len, w_ops, w_opsoff)
    tm = _lib.get_timing()
    res["cigar_stage_device_ms"] = res["best_of_with_cigars"]["device_ms"] - res["best_of_scores_only"]["device_ms"]
    res["summary_over_cigar_stage_device"] = res["summarize_winners"]["device_ms"] / max(res["cigar_stage_device_ms"], 1e-9)
    res["winners"] = int(placed.shape[0])
    res["cigar_runs"] = int(w_ops.shape[0])
    res["columns"] = int(tm["cells"])
    res["gnx_timing_last_call"] = {k: tm[k] for k in TIMING_KEYS}
    res["rescore_equals_score"] = bool((out["rescore"] == scores[placed]).all())
    res["alpha_end_equals_target_end"] = bool((out["alpha_end"] == ends[placed]).all())
    res["mean_identity"] = float(out["n_equal"].sum() / max(int((out["n_equal"] + out["n_mismatch"]).sum()), 1))
    _lib.check(L.gnx_set_reference(None, 0))
    return res


def long_leg(name, args):
    from test_const_long import rescore_const
    from test_long_range import rescore_affine
    affine, a, b = long_pairs.gen(name)
    mx, go, ge = long_pairs.params(affine)
    p = _lib.make_params(_lib.GNX_AFFINE_GAP if affine else _lib.GNX_CONST_GAP, mx, go, ge, 10000, 10000)
    score, ops, off = _lib.align_batch(p, [a], [b])
    host = [None]
    dev = [None]

    def on_host():
        host[0] = rescore_affine(a, b, ops, mx, go, ge) if affine else rescore_const(a, b, ops, mx, go)
        return None

    def on_device():
        dev[0] = _lib.summarize_batch(p, [a], [b], ops, off)[0]
        return _lib.get_timing()["fill_ms"]
    res = alternate({"host_rescore_numpy": on_host, "device_summary": on_device}, args.rounds, args.warmup)
    ni, nj, total = host[0]
    s = dev[0]
    res.update({"case": name, "n": int(a.shape[0]), "m": int(b.shape[0]), "runs": int(ops.shape[0]), "columns": int(ops["run_length"].sum()), "score": int(score[0]),
                "host_rescore": int(total), "device_rescore": int(s["rescore"][0]), "rescores_agree": int(total) == int(s["rescore"][0]),
                "consumed_agree": (int(ni), int(nj)) == (int(s["alpha_used"][0]), int(s["beta_used"][0])),
                "device_over_host_wall": res["device_summary"]["wall_ms"] / res["host_rescore_numpy"]["wall_ms"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--long", default="const_300k_2M,affine_1M", help="cases of tools/long_pairs.py, comma separated; empty: none")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aln_summary.json"))
    args = ap.parse_args()
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    _lib.check(L.gnx_init(0, 0))
    res = {"command": "tools/bench_summary.py " + " ".join(sys.argv[1:]), "rounds": args.rounds, "warmup": args.warmup,
           "reads_workload": "%d reads x %d bases on the synthetic reference (%d bases), max_cand 4, HumanChimpTwo -600 / -150, AffineGapLocal" % (args.reads, READ, args.ref_len)}
    res["reads"] = reads_leg(args)
    res["long_pairs"] = [long_leg(name, args) for name in args.long.split(",") if name]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
