#!/usr/bin/env python
"""The span call (score, target start, target end) against the locate call and against what a caller does today to
learn the start -- the local align call -- in one process, on the same bytes, alternating.

Shape: 100 000 x (query 150 x target 10 000), HumanChimpTwo, -600 / -150, through the windows entries (target = windows of one chunk,
query = the reads, mutated from the chunk: config C2).  Legs: "span" (gnx_locate_span_batch_windows), "locate"
(gnx_locate_batch_windows), "align" (gnx_align_batch_windows, GNX_AFFINE_GAP_LOCAL).  They are warmed up, then timed for --rounds
rounds (>= 9) in which they alternate; per call the kernel time of gnx_get_timing (HIP events) and the wall time of the host entry
(it ends in a device synchronise).  --root names a built tree of the PARENT commit: the locate and align legs then run from that
tree's package and library, loaded beside this one in the same process (the span leg always runs from this tree).  The comparison
that matters is span against the parent's align; locate shows what stage 2 adds.  Prints one JSON line and, with --out, writes it.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_lib_module(root, name):
    """gonomics_amd/_lib.py of another tree under another module name: it binds the library that sits beside it"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "gonomics_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--root", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import common
    from gonomics_amd import _lib, align
    libs = {"span": _lib, "locate": _lib, "align": _lib}
    if args.root:
        parent = _load_lib_module(os.path.abspath(args.root), "gonomics_amd_parent_lib")
        assert os.path.abspath(parent.LIB_PATH) != os.path.abspath(_lib.LIB_PATH)
        libs["locate"] = libs["align"] = parent
    for m in set(libs.values()):
        L = m.lib()
        assert L.gnx_device_count() > 0, "no HIP device"
        m.check(L.gnx_init(0, 0))
    n = args.pairs
    reads, chunk = common.c2_workload(2, n)
    t_start, t_len = np.zeros(n, dtype=np.int64), np.full(n, chunk.shape[0], dtype=np.int64)
    q_start, q_len = np.arange(n, dtype=np.int64) * 150, np.full(n, 150, dtype=np.int64)
    bufs = (chunk, t_start, t_len, reads.reshape(-1), q_start, q_len)
    mx, go, ge = align.HumanChimpTwoScoreMatrix, -600, -150
    params = {m: m.make_params(m.GNX_AFFINE_GAP_LOCAL, mx, go, ge) for m in set(libs.values())}
    cells = int(np.sum(t_len * q_len))
    legs = ["span", "locate", "align"]

    def run(leg):
        m = libs[leg]
        t0 = time.perf_counter()
        if leg == "span":
            out = m.locate_span_batch_windows(params[m], *bufs)
        elif leg == "locate":
            out = m.locate_batch_windows(params[m], *bufs)
        else:
            out = m.align_batch_windows(params[m], *bufs)
        wall = (time.perf_counter() - t0) * 1e3
        tm = m.get_timing()
        return out, wall, tm["total_ms"], tm["dominant_ms"], tm["fast_path"]

    for _ in range(args.warmup):
        outs = {c: run(c) for c in legs}
    # the three legs agree: scores, ends, and the start the align call's CIGAR begins with
    sc, st, en = outs["span"][0]
    assert np.array_equal(sc, outs["locate"][0][0]) and np.array_equal(en, outs["locate"][0][1]), "span != locate"
    a_sc, a_ops, a_off = outs["align"][0]
    first = a_ops[a_off[:-1]]
    a_start = np.where((first["op"] == 2) & (np.diff(a_off) > 1), first["run_length"], 0)
    assert np.array_equal(sc, a_sc) and np.array_equal(st, a_start), "span != align"
    rec = {c: {"wall": [], "kernel": [], "dominant": [], "route": None} for c in legs}
    for _ in range(max(args.rounds, 1)):
        for c in legs:  # the legs alternate
            _, wall, kern, dom, route = run(c)
            rec[c]["wall"].append(wall); rec[c]["kernel"].append(kern); rec[c]["dominant"].append(dom); rec[c]["route"] = route
    res = {"rounds": args.rounds, "warmup": args.warmup, "command": " ".join(["tools/bench_locate_span.py"] + sys.argv[1:]),
           "parent_legs": bool(args.root), "pairs": n, "cells": cells, "mean_span": float(np.mean(en - st)), "legs": {}}
    for c in legs:
        k, wl = sorted(rec[c]["kernel"]), sorted(rec[c]["wall"])
        res["legs"][c] = {"kernel_ms_median": statistics.median(k), "kernel_ms_min": k[0], "kernel_ms_max": k[-1], "kernel_ms": rec[c]["kernel"],
                          "sweep_ms_median": statistics.median(rec[c]["dominant"]),
                          "wall_ms_median": statistics.median(wl), "wall_ms_min": wl[0], "wall_ms_max": wl[-1], "fast_path": rec[c]["route"]}
    lg = res["legs"]
    res["stage2_kernel_ms"] = lg["span"]["kernel_ms_median"] - lg["span"]["sweep_ms_median"]
    res["span_over_align_wall"] = lg["span"]["wall_ms_median"] / lg["align"]["wall_ms_median"]
    res["span_over_locate_wall"] = lg["span"]["wall_ms_median"] / lg["locate"]["wall_ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
