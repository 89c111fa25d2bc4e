#!/usr/bin/env python
"""Score call against align call, same process, same inputs, alternating.

Three shapes: (a) 100 000 x (150 x 10 000), windows entry; (b) 2 000 pairs of 3 000 x 3 000; (c) 64 pairs of 10 000 x 10 000.
Every shape is warmed up, then timed for --rounds rounds (>= 9) in which the two calls alternate; per call the kernel time of
gnx_get_timing (HIP events) and the wall time of the host entry (it ends in a device synchronise).  Prints one JSON line and, with
--out, writes it to a file.  --shapes a,b,c picks shapes; --only score|align runs one of the two calls (for a kernel trace).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# VALU issue floor as bench.py's roofline_valu computes it: instructions per cell / 64 lanes x 1.813 ns per wave-instruction slot and
# SIMD (profiles/r3_valu_ubench4.txt) / (4 SIMDs x 256 CUs)
SLOT_NS, N_SIMD = 1.813, 4 * 256
CELL_INSTR = {"affine": 5, "const": 2}


def shape(name, mode_affine):
    import common
    if name == "a":
        n = 100000
        reads, chunk = common.c2_workload(2, n)
        return dict(a=reads.reshape(-1), a_start=np.arange(n, dtype=np.int64) * 150, a_len=np.full(n, 150, dtype=np.int64), b=chunk,
                    b_start=np.zeros(n, dtype=np.int64), b_len=np.full(n, chunk.shape[0], dtype=np.int64))
    n, ln = (2000, 3000) if name == "b" else (64, 10000)
    rng = np.random.default_rng(7 if name == "b" else 8)
    a = rng.integers(0, 4, size=(n, ln)).astype(np.uint8)
    b = a.copy()
    b[rng.random(b.shape) < 0.08] = 1  # related pairs: 8 % of the positions overwritten
    st = np.arange(n, dtype=np.int64) * ln
    le = np.full(n, ln, dtype=np.int64)
    return dict(a=a.reshape(-1), a_start=st, a_len=le, b=b.reshape(-1), b_start=st.copy(), b_len=le.copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--kind", default="affine", choices=["affine", "const"])
    ap.add_argument("--only", default="", choices=["", "score", "align"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from gonomics_amd import _lib, align
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    _lib.check(L.gnx_init(0, 0))
    mode = _lib.GNX_AFFINE_GAP if args.kind == "affine" else _lib.GNX_CONST_GAP
    p = _lib.make_params(mode, align.HumanChimpTwoScoreMatrix, -600, -150 if args.kind == "affine" else 0)
    res = {"kind": args.kind, "rounds": args.rounds, "warmup": args.warmup, "command": " ".join(["tools/bench_score.py"] + sys.argv[1:]), "shapes": {}}
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    for name in args.shapes.split(","):
        w = shape(name, args.kind == "affine")
        argv = (p, w["a"], w["a_start"], w["a_len"], w["b"], w["b_start"], w["b_len"])
        cells = int(np.sum(w["a_len"] * w["b_len"]))

        def run(which):
            t0 = time.perf_counter()
            out = _lib.score_batch_windows(*argv) if which == "score" else _lib.align_batch_windows(*argv)[0]
            wall = (time.perf_counter() - t0) * 1e3
            tm = _lib.get_timing()
            return out, wall, tm["total_ms"], tm["fast_path"]

        calls = [args.only] if args.only else ["align", "score"]
        for _ in range(args.warmup):
            outs = {c: run(c) for c in calls}
        if len(calls) == 2:
            assert np.array_equal(outs["align"][0], outs["score"][0]), "score call != align call on shape " + name
        rec = {c: {"wall": [], "kernel": [], "route": None} for c in calls}
        for _ in range(max(args.rounds, 1)):
            for c in calls:  # the two calls alternate
                _, wall, kern, route = run(c)
                rec[c]["wall"].append(wall); rec[c]["kernel"].append(kern); rec[c]["route"] = route
        out = {"pairs": int(w["a_len"].shape[0]), "cells": cells}
        for c in calls:
            k, wl = sorted(rec[c]["kernel"]), sorted(rec[c]["wall"])
            out[c] = {"kernel_ms_median": statistics.median(k), "kernel_ms_min": k[0], "kernel_ms_max": k[-1],
                      "wall_ms_median": statistics.median(wl), "wall_ms_min": wl[0], "wall_ms_max": wl[-1], "fast_path": rec[c]["route"],
                      "cells_per_s": cells / (statistics.median(k) * 1e-3)}
        if "score" in out:
            floor_ms = cells * CELL_INSTR[args.kind] / 64.0 * SLOT_NS * 1e-9 / N_SIMD * 1e3
            out["score"]["valu_floor_ms"] = floor_ms
            out["score"]["valu_floor_fraction"] = floor_ms / out["score"]["kernel_ms_median"]
        if len(calls) == 2:
            out["kernel_ratio_align_over_score"] = out["align"]["kernel_ms_median"] / out["score"]["kernel_ms_median"]
            out["wall_ratio_align_over_score"] = out["align"]["wall_ms_median"] / out["score"]["wall_ms_median"]
            out["score_below_align_by_more_than_spread"] = bool(out["score"]["kernel_ms_max"] < out["align"]["kernel_ms_min"] and out["score"]["wall_ms_max"] < out["align"]["wall_ms_min"])
        res["shapes"][name] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
