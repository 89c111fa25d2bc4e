#!/usr/bin/env python
"""Mate pairs in, joint placements out: gnx_best_pair_by_offset against a sequence of older entries.

Workload: tools/bench_map_reads.py's reference, error model and defaults -- the synthetic resident reference, reads of 150 bases with
1 % substitutions and one geometric-length indel in ~26 % of the reads, HumanChimpTwo, -600 / -150, GNX_AFFINE_GAP_LOCAL, a 16-mer
index of every position -- with the reads drawn as MATES: --reads / 2 fragments at uniform positions whose length is normal(--insert-mean,
--insert-sd) clipped to [--insert-lo, --insert-hi]; mate 1 is the fragment's first 150 bases, mate 2 the reverse complement of its last
150; in every other pair the two change places.  Candidates come from gnx_seed_candidates over all mates (not timed here).
Reports, on the same candidate tables:
  best_pair      gnx_best_pair_by_offset: wall clock per call and the device time of its last round (gnx_timing);
  comparator     entries the library had before: gnx_locate_span_batch_by_offset on the flattened list (the reverse complements and
                 the flattened read buffer made with numpy, timed with and without that preparation), the selection rule in numpy,
                 gnx_align_batch_by_offset on the winners (that entry's local roles are the other way round -- the read is its
                 target -- so its CIGARs are not the new call's; its cells are the same);
  agreement      the numpy selection equals the new call's out_best / out_proper / out_tlen exactly;
  placement      the share of pairs placed as proper with both chosen windows over the mates' true origins.
Prints one JSON line and writes it to --out (default profiles/best_pair.json)."""
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

READ = 150


def rc_rows(x):
    x = x[:, ::-1].copy()
    m = x < 4
    x[m] = 3 - x[m]
    return x


def reads_at(rng, pos, ref_seed):
    """reads of 150 bases whose first base is reference position pos[k], with the C3 error model (tests/common.py: c3_reads)"""
    n = pos.shape[0]
    x = np.arange(READ)[None, :]
    has_indel = rng.random(n) < 0.26
    at = rng.integers(10, READ - 10, size=n)
    ln = np.minimum(rng.geometric(0.5, size=n), 32)
    is_del = rng.random(n) < 0.5
    shift = np.where(has_indel[:, None] & (x >= at[:, None]), np.where(is_del, ln, -ln)[:, None], 0)
    src = pos[:, None] + np.clip(x + shift, 0, None)
    reads = _lib.synthetic_reference_positions(src.reshape(-1), ref_seed).reshape(n, READ)
    ins = has_indel[:, None] & (~is_del)[:, None] & (x >= at[:, None]) & (x < (at + ln)[:, None])
    reads = np.where(ins, rng.integers(0, 4, size=reads.shape), reads)
    sub = rng.random(reads.shape) < 0.01
    return np.where(sub, rng.integers(0, 4, size=reads.shape), reads).astype(np.uint8)


def workload(n_pairs, ref_len, seed, mean, sd, lo, hi):
    """reads [2 * n_pairs, 150] (mates adjacent), per read its origin and strand, per pair the fragment length"""
    rng = np.random.default_rng(seed)
    frag = np.clip(np.rint(rng.normal(mean, sd, size=n_pairs)), lo, hi).astype(np.int64)
    o = rng.integers(0, ref_len - hi - 64, size=n_pairs).astype(np.int64)
    fwd, rev = reads_at(rng, o, seed), rc_rows(reads_at(rng, o + frag - READ, seed))
    swap = (np.arange(n_pairs) % 2).astype(bool)
    reads = np.empty((2 * n_pairs, READ), np.uint8)
    reads[0::2], reads[1::2] = np.where(swap[:, None], rev, fwd), np.where(swap[:, None], fwd, rev)
    origin, strand = np.empty(2 * n_pairs, np.int64), np.empty(2 * n_pairs, np.uint8)
    origin[0::2], origin[1::2] = np.where(swap, o + frag - READ, o), np.where(swap, o, o + frag - READ)
    strand[0::2], strand[1::2] = swap, ~swap
    return np.ascontiguousarray(reads), origin, strand, frag


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "ms": ms}


def numpy_selection(c_off, c_start, c_strand, score, start, end, lo, hi, pen, kmax):
    """the selection rule of gnx_best_pair_* over padded [pairs, kmax] tables: (best per read, proper, tlen)"""
    n = c_off.shape[0] - 1
    cnt = np.diff(c_off)
    slot = np.arange(kmax)[None, :]
    valid = slot < cnt[:, None]
    idx = np.minimum(c_off[:-1, None] + slot, max(score.shape[0] - 1, 0))
    neg = np.iinfo(np.int64).min // 4
    sc = np.where(valid, score[idx], neg)
    a, e, st = c_start[idx] + start[idx], c_start[idx] + end[idx], c_strand[idx]
    nonempty = valid & (end[idx] > start[idx])
    first = np.where(cnt > 0, np.argmax(sc, axis=1), -1)
    s1, s2, a1, a2, e1, e2 = sc[0::2, :, None], sc[1::2, None, :], a[0::2, :, None], a[1::2, None, :], e[0::2, :, None], e[1::2, None, :]
    t1, t2 = st[0::2, :, None], st[1::2, None, :]
    af, ef, av, ev = np.where(t1 == 0, a1, a2), np.where(t1 == 0, e1, e2), np.where(t1 == 0, a2, a1), np.where(t1 == 0, e2, e1)
    tl = ev - af
    ok = nonempty[0::2, :, None] & nonempty[1::2, None, :] & (t1 != t2) & (af <= av) & (ef <= ev) & (tl >= lo) & (tl <= hi)
    ps = np.where(ok, s1 + s2, neg).reshape(n // 2, kmax * kmax)
    top = np.argmax(ps, axis=1)
    rows = np.arange(n // 2)
    u = np.where(first[0::2] >= 0, sc[0::2][rows, first[0::2]], 0) + np.where(first[1::2] >= 0, sc[1::2][rows, first[1::2]], 0) - pen
    proper = ok.reshape(n // 2, -1)[rows, top] & (ps[rows, top] >= u)
    best = first.copy()
    best[0::2] = np.where(proper, top // kmax, first[0::2])
    best[1::2] = np.where(proper, top % kmax, first[1::2])
    return best.astype(np.int32), proper.astype(np.uint8), np.where(proper, tl.reshape(n // 2, -1)[rows, top], 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--seed-len", type=int, default=16)
    ap.add_argument("--seed-step", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--insert-mean", type=float, default=400)
    ap.add_argument("--insert-sd", type=float, default=50)
    ap.add_argument("--insert-lo", type=int, default=250)
    ap.add_argument("--insert-hi", type=int, default=600)
    ap.add_argument("--min-insert", type=int, default=200)
    ap.add_argument("--max-insert", type=int, default=700)
    ap.add_argument("--unpaired-penalty", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_pair.json"))
    for k, v in align.SEED_VOTE_DEFAULTS.items():
        ap.add_argument("--" + k.replace("_", "-"), type=int, default=v)
    args = ap.parse_args()
    vote = {k: getattr(args, k) for k in align.SEED_VOTE_DEFAULTS}
    n = args.reads - args.reads % 2
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    _lib.check(L.gnx_init(0, 0))
    _lib.check(L.gnx_set_reference_synthetic(args.ref_len, args.seed))
    _lib.reference_index_build(args.seed_len, args.seed_step)
    reads, origin, strand, frag = workload(n // 2, args.ref_len, args.seed, args.insert_mean, args.insert_sd, args.insert_lo, args.insert_hi)
    r_cat, r_off = reads.reshape(-1), np.arange(n + 1, dtype=np.int64) * READ
    c_off, c_start, c_len, c_strand, _ = _lib.seed_candidates(r_cat, r_off, **vote)
    nc = int(c_off[-1])
    res = {"workload": "%d mate pairs x 2 x %d bases (1 %% substitutions, an indel in ~26 %%), fragments normal(%g, %g) clipped to [%d, %d], the reverse mate first in every other pair, "
                       "on the synthetic reference (%d bases), HumanChimpTwo -600 / -150, AffineGapLocal" % (n // 2, READ, args.insert_mean, args.insert_sd, args.insert_lo, args.insert_hi, args.ref_len),
           "command": "tools/bench_best_pair.py " + " ".join(sys.argv[1:]), "rounds": args.rounds, "vote_opts": vote, "candidates": nc,
           "pair_opts": {"min_insert": args.min_insert, "max_insert": args.max_insert, "unpaired_penalty": args.unpaired_penalty}}
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
    o = _lib.pair_opts(args.min_insert, args.max_insert, args.unpaired_penalty)
    keys = ("fast_path", "fill_ms", "dominant_ms", "total_ms", "host_ms", "cells", "n_launches")

    # ---- the new call ----
    new = _lib.best_pair_by_offset(p, o, r_cat, r_off, c_off, c_start, c_len, c_strand)  # warm-up: buffers
    ms, dev = [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        new = _lib.best_pair_by_offset(p, o, r_cat, r_off, c_off, c_start, c_len, c_strand)
        ms.append((time.perf_counter() - t0) * 1e3)
        dev.append(_lib.get_timing()["total_ms"])
    tm = _lib.get_timing()
    res["best_pair"] = dict(spread(ms), device_total_ms_median=statistics.median(dev), gnx_timing_last_round={k: tm[k] for k in keys})

    # ---- the comparator: span entry on the flattened list, selection in numpy, align entry on the winners ----
    read_of = np.repeat(np.arange(n), np.diff(c_off))

    def flatten():
        q = reads[read_of]
        back = c_strand == 1
        q[back] = rc_rows(q[back])
        return q.reshape(-1), np.arange(nc + 1, dtype=np.int64) * READ

    def comparator(flat):
        t = [time.perf_counter()]
        q_cat, q_off = flat if flat is not None else flatten()
        t.append(time.perf_counter())
        sc, st, en = _lib.locate_span_batch_by_offset(p, q_cat, q_off, c_start, c_len)
        d_span = _lib.get_timing()["total_ms"]
        t.append(time.perf_counter())
        best, proper, tlen = numpy_selection(c_off, c_start, c_strand, sc, st, en, args.min_insert, args.max_insert, args.unpaired_penalty, vote["max_cand"])
        t.append(time.perf_counter())
        placed = best >= 0
        w = c_off[:-1][placed] + best[placed]
        a_sc, a_ops, a_off = _lib.align_batch_by_offset(p, q_cat.reshape(-1, READ)[w].reshape(-1), np.arange(w.shape[0] + 1, dtype=np.int64) * READ, c_start[w], c_len[w])
        d_align = _lib.get_timing()["total_ms"]
        t.append(time.perf_counter())
        return np.diff(t) * 1e3, d_span + d_align, (best, proper, tlen)

    comparator(None)  # warm-up
    flat = flatten()
    parts, dev, without = [], [], []
    for _ in range(args.rounds):
        ms_parts, d, sel = comparator(None)
        parts.append(ms_parts.tolist())
        dev.append(d)
        without.append(float(comparator(flat)[0][1:].sum()))
    parts = np.asarray(parts)
    res["comparator"] = dict(spread(parts.sum(axis=1).tolist()), device_total_ms_median=statistics.median(dev),
                             median_ms_by_step={k: float(np.median(parts[:, x])) for x, k in enumerate(("flatten_numpy", "locate_span_by_offset", "selection_numpy", "align_by_offset_winners"))},
                             without_flatten=spread(without),
                             entries=["gnx_locate_span_batch_by_offset", "numpy selection", "gnx_align_batch_by_offset"])
    res["best_pair_over_comparator_wall"] = res["best_pair"]["median_ms"] / res["comparator"]["median_ms"]
    res["best_pair_over_comparator_wall_without_flatten"] = res["best_pair"]["median_ms"] / res["comparator"]["without_flatten"]["median_ms"]
    res["best_pair_over_comparator_device"] = res["best_pair"]["device_total_ms_median"] / max(res["comparator"]["device_total_ms_median"], 1e-9)
    best, proper, tlen = sel
    res["numpy_selection_equals_the_call"] = bool(np.array_equal(best, new["best"]) and np.array_equal(proper, new["proper"]) and np.array_equal(tlen, new["tlen"]))

    # ---- placement ----
    placed = new["best"] >= 0
    w = c_off[:-1] + np.maximum(new["best"], 0)
    w = np.minimum(w, max(nc - 1, 0))
    over = placed & (c_strand[w] == strand) & (c_start[w] <= origin) & (origin < c_start[w] + c_len[w])
    both = over[0::2] & over[1::2]
    res["share_of_pairs_placed_as_proper"] = float(new["proper"].mean())
    res["share_of_pairs_placed_as_proper_over_their_true_origin"] = float((both & (new["proper"] == 1)).mean())
    res["share_of_pairs_with_both_mates_over_their_true_origin"] = float(both.mean())
    res["median_abs_tlen_error"] = float(np.median(np.abs(new["tlen"][new["proper"] == 1] - frag[new["proper"] == 1]))) if new["proper"].any() else None
    _lib.check(L.gnx_set_reference(None, 0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
