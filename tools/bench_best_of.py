#!/usr/bin/env python
"""Best-of-K read placement on both strands: the one-call entry (gnx_best_of_by_offset) against the two-call sequence the same
library offers without it, one process, alternating.

Workload: --reads reads of 150 bases (20 000), K = 4 candidate windows of 1 000 bases of the synthetic resident reference
(gnx_set_reference_synthetic), one of them over the read's origin, half of the reads sequenced from the other strand and half of all
candidates on strand 1; HumanChimpTwo, -600 / -150; global affine (GNX_AFFINE_GAP) and the mapping mode (GNX_AFFINE_GAP_LOCAL).
  new       _lib.best_of_by_offset: reads uploaded once, reverse complements / selection / winners' tables on the device
  baseline  reverse complement on the host and one read copy per candidate, score_batch_by_offset (local: locate_batch_by_offset),
            first maximum on the host, align_batch_by_offset for the winners (local: align_batch_windows, alpha = the winners' windows
            gathered from a host copy of the reference)
Both legs are checked against each other once (winners, scores, CIGARs, ends), then alternate for --rounds rounds after --warmup.
Per leg: wall-clock median, min and max in ms; for the new call also the gnx_timing of its last round.  Prints one JSON line and
writes it to --out (default profiles/best_of.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gonomics_amd import _lib, align  # noqa: E402

READ, WINDOW, K = 150, 1000, 4


def revcomp_rows(reads):
    out = reads[:, ::-1].copy()
    m = out < 4
    out[m] = 3 - out[m]
    return out


def workload(n_reads, ref_len, seed):
    """reads [n, 150] (1 % substitutions; odd reads from the other strand), window starts / strands [n, 4], a host copy of every window"""
    rng = np.random.default_rng(seed)
    origin = rng.integers(WINDOW, ref_len - 2 * WINDOW, size=n_reads)
    reads = _lib.synthetic_reference_positions((origin[:, None] + np.arange(READ)[None, :]).reshape(-1), seed).reshape(n_reads, READ)
    sub = rng.random(reads.shape) < 0.01
    reads[sub] = (reads[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
    strand = (np.arange(n_reads) % 2).astype(np.uint8)
    reads[strand == 1] = revcomp_rows(reads[strand == 1])
    starts = rng.integers(0, ref_len - WINDOW, size=(n_reads, K))
    strands = np.stack([strand, 1 - strand, strand, 1 - strand], axis=1).astype(np.uint8)  # half of the candidates on strand 1
    true_at = 2 * rng.integers(0, 2, size=n_reads)                                         # (a slot with the read's own strand)
    starts[np.arange(n_reads), true_at] = origin - rng.integers(0, WINDOW - READ, size=n_reads)
    windows = _lib.synthetic_reference_positions((starts.reshape(-1)[:, None] + np.arange(WINDOW)[None, :]).reshape(-1), seed).reshape(n_reads * K, WINDOW)
    return np.ascontiguousarray(reads, np.uint8), starts.astype(np.int64), strands, windows


def leg_new(p, w):
    reads, starts, strands, _ = w
    n = reads.shape[0]
    return _lib.best_of_by_offset(p, reads.reshape(-1), np.arange(n + 1, dtype=np.int64) * READ, np.arange(n + 1, dtype=np.int64) * K,
                                  starts.reshape(-1), np.full(n * K, WINDOW, np.int64), strands.reshape(-1))


def leg_baseline(p, w):
    reads, starts, strands, windows = w
    n = reads.shape[0]
    local = p.mode == _lib.GNX_AFFINE_GAP_LOCAL
    rc = revcomp_rows(reads)                                                     # dna.ReverseComplement of every read, on the host
    rep = np.where(strands.reshape(-1)[:, None] == 1, np.repeat(rc, K, axis=0), np.repeat(reads, K, axis=0))  # one read copy per candidate
    off = np.arange(n * K + 1, dtype=np.int64) * READ
    lens = np.full(n * K, WINDOW, np.int64)
    if local:
        cand, cand_end = _lib.locate_batch_by_offset(p, rep.reshape(-1), off, starts.reshape(-1), lens)
    else:
        cand, cand_end = _lib.score_batch_by_offset(p, rep.reshape(-1), off, starts.reshape(-1), lens), None
    best = np.argmax(cand.reshape(n, K), axis=1)                                 # the first maximum
    win = np.arange(n) * K + best
    q = np.ascontiguousarray(rep[win])
    q_off = np.arange(n + 1, dtype=np.int64) * READ
    if local:
        t = np.ascontiguousarray(windows[win])                                   # the winners' windows as bytes: AffineGapLocal(target = window, query = read)
        sc, ops, o = _lib.align_batch_windows(p, t.reshape(-1), np.arange(n, dtype=np.int64) * WINDOW, lens[:n], q.reshape(-1), q_off[:-1], np.full(n, READ, np.int64))
    else:
        sc, ops, o = _lib.align_batch_by_offset(p, q.reshape(-1), q_off, starts.reshape(-1)[win], lens[:n])
    return best.astype(np.int32), sc, (cand_end[win] if local else None), cand, ops, o


def same(a, b):
    ok = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and np.array_equal(a[5], b[5])
    ok = ok and np.array_equal(a[4]["run_length"], b[4]["run_length"]) and np.array_equal(a[4]["op"], b[4]["op"])
    return bool(ok and (a[2] is None) == (b[2] is None) and (a[2] is None or np.array_equal(a[2], b[2])))


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_of.json"))
    args = ap.parse_args()
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    _lib.check(L.gnx_init(0, 0))
    _lib.check(L.gnx_set_reference_synthetic(args.ref_len, args.seed))
    w = workload(args.reads, args.ref_len, args.seed)
    res = {"workload": "%d reads x %d bases, K = %d windows of %d bases of the synthetic reference (%d bases), half of the candidates on strand 1, HumanChimpTwo -600 / -150"
                       % (args.reads, READ, K, WINDOW, args.ref_len),
           "command": "tools/bench_best_of.py --reads %d --ref-len %d --seed %d --rounds %d --warmup %d" % (args.reads, args.ref_len, args.seed, args.rounds, args.warmup),
           "rounds": args.rounds, "warmup": args.warmup, "modes": {}}
    for name, mode in (("global_affine", _lib.GNX_AFFINE_GAP), ("local", _lib.GNX_AFFINE_GAP_LOCAL)):
        p = _lib.make_params(mode, align.HumanChimpTwoScoreMatrix, -600, -150)
        a, b = leg_new(p, w), leg_baseline(p, w)
        rec = {"results_identical": same(a, b), "reverse_strand_winners": int(np.sum(w[2][np.arange(args.reads), a[0]] == 1)), "cigar_runs": int(a[5][-1])}
        for _ in range(max(args.warmup - 1, 0)):
            leg_new(p, w)
            leg_baseline(p, w)
        ms = {"new": [], "baseline": []}
        timing = {}
        for _ in range(max(args.rounds, 1)):  # the legs alternate
            t0 = time.perf_counter()
            leg_new(p, w)
            ms["new"].append((time.perf_counter() - t0) * 1e3)
            timing = _lib.get_timing()
            t0 = time.perf_counter()
            leg_baseline(p, w)
            ms["baseline"].append((time.perf_counter() - t0) * 1e3)
        rec["new"], rec["baseline"] = spread(ms["new"]), spread(ms["baseline"])
        rec["new"]["gnx_timing_last_round"] = {k: timing[k] for k in ("fast_path", "fill_ms", "dominant_ms", "total_ms", "host_ms", "fetch_ms", "cells", "n_launches")}
        rec["new_over_baseline"] = rec["new"]["median_ms"] / rec["baseline"]["median_ms"]
        rec["new_exceeds_baseline_by_more_than_its_spread"] = bool(rec["new"]["median_ms"] - rec["baseline"]["median_ms"] > rec["baseline"]["max_ms"] - rec["baseline"]["min_ms"])
        res["modes"][name] = rec
    _lib.check(L.gnx_set_reference(None, 0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
