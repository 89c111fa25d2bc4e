#!/usr/bin/env python
"""Score-first progressive alignment against the driver that aligns every pair every round, one process, alternating.

Workload: cmd/faChunkAlign of DESIGN.md 5.1 -- 8 sequences x 30 kb, chunk 3, HumanChimpTwo, -300 / -40 (tools/bench_n1_cmd.py's records),
multi-fasta in, multi-fasta out.  --root names a second tree (the parent commit, built beside this one): its gonomics_amd package and
its built library are loaded into the SAME process under another name, and the two commands alternate for --rounds rounds (>= 9)
after --warmup.  Per command: wall time, the DP kernel time (fill_ms of gnx_get_timing summed over its device calls), the number of
pairs scored and aligned; per tree the device memory its first command allocated (hipMemGetInfo before and after: buffers are kept).
One more leg, this tree only: the 28 first-round pairs alone, score entry against align entry.  Prints one JSON line; --out writes it.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def load_tree(root, name):
    """the gonomics_amd package of `root` under the module name `name` (its relative imports and its library path stay its own)"""
    if os.path.abspath(root) == ROOT:
        import gonomics_amd
        return gonomics_amd
    pkg = os.path.join(os.path.abspath(root), "gonomics_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def free_bytes(hip):
    fr, tot = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(fr), ctypes.byref(tot)) == 0
    return int(fr.value)


class Tree:
    def __init__(self, label, pkg):
        self.label = label
        self._lib = importlib.import_module(pkg.__name__ + "._lib")
        self.align = importlib.import_module(pkg.__name__ + ".align")
        self.cmds = importlib.import_module(pkg.__name__ + ".cmds")
        self.fasta = importlib.import_module(pkg.__name__ + ".fasta")
        L = self._lib.lib()
        assert L.gnx_device_count() > 0, "no HIP device"
        self._lib.check(L.gnx_init(0, 0))
        self.calls = []
        for fn in ("multiple_affine_gap_batch", "multiple_affine_gap_score_batch"):
            if hasattr(self._lib, fn):
                setattr(self._lib, fn, self._timed(fn, getattr(self._lib, fn)))

    def _timed(self, name, inner):
        def call(params, chunk, groups, pairs):
            t0 = time.perf_counter()
            out = inner(params, chunk, groups, pairs)
            tm = self._lib.get_timing()
            self.calls.append({"entry": name, "pairs": len(pairs), "call_ms": (time.perf_counter() - t0) * 1e3, "fill_ms": tm["fill_ms"], "traceback_ms": tm["traceback_ms"], "fast_path": tm["fast_path"]})
            return out
        return call

    def command(self, fin, fout, chunk, go, ge):
        self.calls = []
        t0 = time.perf_counter()
        self.cmds.faChunkAlign(fin, chunk, go, ge, fout)
        wall = time.perf_counter() - t0
        return {"command_s": wall, "dp_kernel_ms": sum(c["fill_ms"] for c in self.calls), "traceback_kernel_ms": sum(c["traceback_ms"] for c in self.calls),
                "pairs_scored": sum(c["pairs"] for c in self.calls if c["entry"].endswith("score_batch")),
                "pairs_aligned": sum(c["pairs"] for c in self.calls if not c["entry"].endswith("score_batch")),
                "routes": sorted({c["fast_path"] for c in self.calls}), "calls": list(self.calls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default="", help="a second tree (the parent commit, built) measured in the same process")
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--bases", type=int, default=30000)
    ap.add_argument("--chunk", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench_n1_cmd
    os.environ["GNX_N1_SCORE_FIRST"] = "1"  # this tree runs score first (read per call by align._all_seq); the parent's driver does not know the switch
    go, ge = -300, -40
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    trees = [Tree("this", load_tree(ROOT, "gonomics_amd"))]
    if args.root:
        trees.append(Tree("parent", load_tree(args.root, "gonomics_amd_parent")))
    recs = bench_n1_cmd.make_records(args.seqs, args.bases, args.chunk)
    tmp = tempfile.mkdtemp()
    fin = os.path.join(tmp, "in.fa")
    trees[0].fasta.Write(fin, recs)
    res = {"workload": "cmd/faChunkAlign: %d sequences x %d bases, chunk %d, HumanChimpTwo, gapOpen %d gapExtend %d" % (args.seqs, args.bases, args.chunk, go, ge),
           "command": " ".join(["tools/bench_n1_score.py"] + sys.argv[1:]), "rounds": args.rounds, "warmup": args.warmup, "trees": {}}
    outs = {}
    for t in trees:  # first use: what the command allocates on the device
        before = free_bytes(hip)
        first = t.command(fin, os.path.join(tmp, t.label + ".fa"), args.chunk, go, ge)
        res["trees"][t.label] = {"lib": os.path.relpath(t._lib.LIB_PATH, ROOT), "first_use_device_bytes": before - free_bytes(hip), "first_command_s": first["command_s"],
                                 "pairs_scored": first["pairs_scored"], "pairs_aligned": first["pairs_aligned"], "routes": first["routes"]}
        outs[t.label] = open(os.path.join(tmp, t.label + ".fa"), "rb").read()
    res["outputs_identical"] = len(set(outs.values())) == 1
    for _ in range(max(args.warmup - 1, 0)):
        for t in trees:
            t.command(fin, os.path.join(tmp, t.label + ".fa"), args.chunk, go, ge)
    rec = {t.label: [] for t in trees}
    for _ in range(max(args.rounds, 1)):
        for t in trees:  # the trees alternate
            rec[t.label].append(t.command(fin, os.path.join(tmp, t.label + ".fa"), args.chunk, go, ge))
    for t in trees:
        r = rec[t.label]
        d = res["trees"][t.label]
        d["command_s_median"] = statistics.median(x["command_s"] for x in r)
        d["command_s"] = [x["command_s"] for x in r]
        d["dp_kernel_ms_median"] = statistics.median(x["dp_kernel_ms"] for x in r)
        d["dp_kernel_ms"] = [x["dp_kernel_ms"] for x in r]
        d["traceback_kernel_ms_median"] = statistics.median(x["traceback_kernel_ms"] for x in r)
        d["last_round_calls"] = r[-1]["calls"]
    if len(trees) == 2:
        res["command_speedup"] = res["trees"]["parent"]["command_s_median"] / res["trees"]["this"]["command_s_median"]
    # the 28 first-round pairs alone: score entry against align entry (this tree)
    t = trees[0]
    blocks = [np.asarray(r.Seq, dtype=np.uint8)[None, :] for r in recs]
    prs = [(x, y) for x in range(len(blocks) - 1) for y in range(x + 1, len(blocks))]
    p = t._lib.make_params(t._lib.GNX_AFFINE_GAP_HIGHMEM, t.align.HumanChimpTwoScoreMatrix, go, ge)
    legs = {"score": [], "align": []}
    same = True
    for k in range(args.warmup + args.rounds):
        t.calls = []
        sc = t._lib.multiple_affine_gap_score_batch(p, args.chunk, blocks, prs)
        sa = t._lib.multiple_affine_gap_batch(p, args.chunk, blocks, prs)[0]
        same = same and bool(np.array_equal(sc, sa))
        if k >= args.warmup:
            legs["score"].append(t.calls[0]); legs["align"].append(t.calls[1])
    cells = sum(blocks[x].shape[1] // args.chunk * (blocks[y].shape[1] // args.chunk) for x, y in prs)
    res["first_round_alone"] = {"pairs": len(prs), "chunk_cells": cells, "scores_equal": same}
    for leg, cs in legs.items():
        res["first_round_alone"][leg] = {"call_ms_median": statistics.median(c["call_ms"] for c in cs), "dp_kernel_ms_median": statistics.median(c["fill_ms"] for c in cs),
                                         "traceback_kernel_ms_median": statistics.median(c["traceback_ms"] for c in cs), "fast_path": cs[-1]["fast_path"],
                                         "cells_per_s_kernel": cells / (statistics.median(c["fill_ms"] for c in cs) * 1e-3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
