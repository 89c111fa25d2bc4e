#!/usr/bin/env python
"""The local (AffineGapLocal) score and locate calls against the local align call and the global score call, same process, same
bytes, alternating.

Shape: 100 000 x (query 150 x target 10 000), HumanChimpTwo, -600 / -150, through the windows entries (alpha = target = windows of
one chunk, beta = query = the reads).  The legs -- local score, local locate, local align, global score -- are warmed up, then timed
for --rounds rounds (>= 9) in which they alternate; per call the kernel time of gnx_get_timing (HIP events) and the wall time of the
host entry (it ends in a device synchronise).  Prints one JSON line and, with --out, writes it to a file.
--legs picks legs (a build without the locate entries runs "score,align,global"); --root names the tree whose gonomics_amd package
and built library are used (default: this one), so that the parent commit, built beside this one, is measured with the same tool.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# VALU issue floor as bench.py's roofline_valu computes it: instructions per cell / 64 lanes x 1.813 ns per wave-instruction slot and
# SIMD (profiles/r3_valu_ubench4.txt) / (4 SIMDs x 256 CUs); the local cell is the global affine one: add, max3, add, max, max
SLOT_NS, N_SIMD, CELL_INSTR = 1.813, 4 * 256, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--legs", default="score,locate,align,global")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import common
    from gonomics_amd import _lib, align
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    _lib.check(L.gnx_init(0, 0))
    n = args.pairs
    reads, chunk = common.c2_workload(2, n)
    t_start, t_len = np.zeros(n, dtype=np.int64), np.full(n, chunk.shape[0], dtype=np.int64)
    q_start, q_len = np.arange(n, dtype=np.int64) * 150, np.full(n, 150, dtype=np.int64)
    bufs = (chunk, t_start, t_len, reads.reshape(-1), q_start, q_len)
    mx, go, ge = align.HumanChimpTwoScoreMatrix, -600, -150
    p_local = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
    p_global = _lib.make_params(_lib.GNX_AFFINE_GAP, mx, go, ge)
    cells = int(np.sum(t_len * q_len))
    legs = args.legs.split(",")

    def run(leg):
        t0 = time.perf_counter()
        if leg == "score":
            out = _lib.score_batch_windows(p_local, *bufs)
        elif leg == "locate":
            out = _lib.locate_batch_windows(p_local, *bufs)[0]
        elif leg == "align":
            out = _lib.align_batch_windows(p_local, *bufs)[0]
        else:
            out = _lib.score_batch_windows(p_global, *bufs)
        wall = (time.perf_counter() - t0) * 1e3
        tm = _lib.get_timing()
        return out, wall, tm["total_ms"], tm["fast_path"]

    for _ in range(args.warmup):
        outs = {c: run(c) for c in legs}
    for c in ("score", "locate"):
        if c in outs and "align" in outs:
            assert np.array_equal(outs[c][0], outs["align"][0]), c + " call != align call"
    rec = {c: {"wall": [], "kernel": [], "route": None} for c in legs}
    for _ in range(max(args.rounds, 1)):
        for c in legs:  # the legs alternate
            _, wall, kern, route = run(c)
            rec[c]["wall"].append(wall); rec[c]["kernel"].append(kern); rec[c]["route"] = route
    res = {"rounds": args.rounds, "warmup": args.warmup, "command": " ".join(["tools/bench_score_local.py"] + sys.argv[1:]), "lib": os.path.relpath(_lib.LIB_PATH, ROOT),
           "pairs": n, "cells": cells, "legs": {}}
    for c in legs:
        k, wl = sorted(rec[c]["kernel"]), sorted(rec[c]["wall"])
        res["legs"][c] = {"kernel_ms_median": statistics.median(k), "kernel_ms_min": k[0], "kernel_ms_max": k[-1], "kernel_ms": rec[c]["kernel"],
                          "wall_ms_median": statistics.median(wl), "wall_ms_min": wl[0], "wall_ms_max": wl[-1], "fast_path": rec[c]["route"],
                          "cells_per_s": cells / (statistics.median(k) * 1e-3)}
    floor_ms = cells * CELL_INSTR / 64.0 * SLOT_NS * 1e-9 / N_SIMD * 1e3
    res["valu_floor_ms"] = floor_ms
    for c in ("score", "locate"):
        if c in res["legs"]:
            res["legs"][c]["valu_floor_fraction"] = floor_ms / res["legs"][c]["kernel_ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
