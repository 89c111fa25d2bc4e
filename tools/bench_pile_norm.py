#!/usr/bin/env python
"""Left-normalised alleles of the pile (gnx_pileup_alleles_norm): what normalising costs a query, and what the wave
phase of norm_shift_kernel buys on an adversarial repeat.

  (a) the workload of DESIGN.md 4.26 as tools/bench_pile_alleles.py builds it (--reads reads of 150 bases on the synthetic resident
      reference, the winners added to a tracking pile over the whole reference): `alleles` (the plain query) and `alleles_norm` (the
      normalised one) alternating in one process, medians of --rounds rounds after --warmup warm-ups, every round on a fresh pile.  A
      library without the normalised entry (the parent commit's, loaded through GNX_LIB_PATH) runs the plain leg alone, in the same
      sequence of calls.
  (b) an adversarial pile built here: a reference with an exact period-7 repeat of --repeat bases and --repeat-reads reads that each
      delete one unit at its right end, so every event shifts by the whole repeat (`dense`); and the same pile with only one read in
      64 there and the others in a repeat of two units (`sparse`: a wave holds about one long event).  The normalised query with
      GNX_NORM_COOP 0 (every lane finishes alone) and 1 (the wave takes long events over), alternating.
Device time is gnx_timing.fill_ms, kernel time gnx_timing.dominant_ms (the normalised query: norm_shift_kernel alone).  The normalised
alleles of --check winners of (a) and all of (b) are compared with the restatement (tests/pyref_pile_norm.py).  Prints one JSON line
and writes it to --out (default profiles/pile_norm.json; "" = nowhere)."""
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


def _listed(arr):
    return [(int(a["pos"]), int(a["kind"]), int(a["seq"]) if a["kind"] == 2 else int(a["length"]), int(a["count"]), int(a["count_fwd"])) for a in arr]


def _stats(wall, dev, kern, skip):
    w, d, k = wall[skip:], dev[skip:], kern[skip:]
    return {"wall_ms": statistics.median(w), "device_ms": statistics.median(d), "device_min_ms": min(d), "device_max_ms": max(d), "kernel_ms": statistics.median(k),
            "kernel_min_ms": min(k), "kernel_max_ms": max(k)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--ref-len", type=int, default=64000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=300, help="winners of (a) whose normalised alleles are compared with the restatement")
    ap.add_argument("--repeat", type=int, default=100000, help="(b): bases of the exact period-7 repeat")
    ap.add_argument("--repeat-reads", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pile_norm.json"))
    args = ap.parse_args()
    L = _lib.lib()
    assert L.gnx_device_count() > 0, "no HIP device"
    has_norm = hasattr(L, "gnx_pileup_alleles_norm")
    _lib.check(L.gnx_init(0, 0))
    series = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        t = _lib.get_timing()
        s = series.setdefault(name, ([], [], []))
        s[0].append(wall)
        s[1].append(t["fill_ms"])
        s[2].append(t["dominant_ms"])
        return out

    res = {"command": "tools/bench_pile_norm.py " + " ".join(sys.argv[1:]), "library": os.path.basename(_lib.LIB_PATH), "library_normalises": has_norm,
           "rounds": args.rounds, "warmup": args.warmup,
           "device_ms_is": "gnx_timing.fill_ms; kernel_ms is gnx_timing.dominant_ms (the normalised query: norm_shift_kernel alone)"}
    # ---- (a) ----
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
    for r in range(args.warmup + args.rounds):
        _lib.pileup_open(0, args.ref_len)
        _lib.pileup_track_alleles(0)
        _lib.pileup_add_by_offset(p, w_cat, w_off, win_start, win_len, strand, w_ops, w_opsoff)
        res["a_events"] = _lib.pileup_allele_info()["events"]
        res["a_alleles"] = int(timed("a_alleles", _lib.pileup_alleles).shape[0])
        if has_norm:
            res["a_alleles_norm"] = int(timed("a_alleles_norm", lambda: _lib.pileup_alleles(normalize=True)).shape[0])
    res["a_winners"] = int(placed.shape[0])
    res["a"] = {k[2:]: _stats(*v, args.warmup) for k, v in series.items() if k.startswith("a_")}
    if has_norm:
        res["a"]["norm_extra_device_ms"] = res["a"]["alleles_norm"]["device_ms"] - res["a"]["alleles"]["device_ms"]
        import pyref_pile_norm
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

        class Codes:  # the reference codes around the checked alleles, fetched in pieces
            def __init__(self):
                self.blocks = {}

            def __getitem__(self, x):
                b = x >> 12
                if b not in self.blocks:
                    self.blocks[b] = _lib.synthetic_reference_bases(b << 12, min(4096, args.ref_len - (b << 12)), args.seed)
                return int(self.blocks[b][x & 4095])

        res["a_checked_against_restatement"] = k
        res["a_restatement_agrees"] = bool(_listed(_lib.pileup_alleles(normalize=True)) == pyref_pile_alleles.listed(pyref_pile_norm.normalized(want, Codes(), (0, args.ref_len))))
        # ---- (b) ----
        rng = np.random.default_rng(args.seed)
        flank = 200
        unit = np.array([0, 1, 1, 2, 3, 0, 2], dtype=np.uint8)
        rep = np.resize(unit, args.repeat)
        # flank, the long repeat, flank, two units (a deletion of one shifts by 7 there), flank
        g = np.concatenate([rng.integers(0, 4, size=flank).astype(np.uint8), rep, rng.integers(0, 4, size=flank).astype(np.uint8), np.resize(unit, 14),
                            rng.integers(0, 4, size=flank).astype(np.uint8)])
        x = flank + args.repeat - 7      # the long repeat's last unit
        xs = 2 * flank + args.repeat + 7  # the short one's
        for first in (flank, xs - 7):
            g[first - 1] = (g[first - 1 + 7] + 1) % 4
        _lib.set_reference(g)
        route = np.zeros(3, dtype=_lib.CIGAR_DTYPE)
        route["run_length"], route["op"] = [60, 7, 60], [align.ColM, align.ColD, align.ColM]
        nb = args.repeat_reads
        b_off = np.arange(nb + 1, dtype=np.int64) * 120
        b_ops, b_opsoff = np.tile(route, nb), np.arange(nb + 1, dtype=np.int64) * 3
        b_len = np.full(nb, 127, dtype=np.int64)
        b_strand = (np.arange(nb) % 2).astype(np.uint8)
        before = os.environ.get("GNX_NORM_COOP")
        try:
            # dense: every event is long.  sparse: one read in 64 deletes in the long repeat, the others in the short one
            for leg, every in (("b_dense", 1), ("b_sparse", 64)):
                at = np.where(np.arange(nb) % every == 0, x, xs).astype(np.int64)
                b_cat = np.concatenate([np.concatenate([g[q - 60:q], g[q + 7:q + 67]]) for q in at])
                n_long = int((at == x).sum())
                fwd_long = int(((at == x) & (b_strand == 0)).sum())
                want = [(flank, 1, 7, n_long, fwd_long)] + ([(xs - 7, 1, 7, nb - n_long, (nb + 1) // 2 - fwd_long)] if n_long < nb else [])
                for r in range(args.warmup + args.rounds):
                    _lib.pileup_open(0, g.shape[0])
                    _lib.pileup_track_alleles(0)
                    _lib.pileup_add_by_offset(p, b_cat, b_off, at - 60, b_len, b_strand, b_ops, b_opsoff)
                    for coop in ("0", "1"):
                        os.environ["GNX_NORM_COOP"] = coop
                        got = _listed(timed("%s_coop%s" % (leg, coop), lambda: _lib.pileup_alleles(normalize=True)))
                        res["%s_agrees_coop%s" % (leg, coop)] = bool(got == want)
                res[leg + "_long_events"] = n_long
        finally:
            if before is None:
                os.environ.pop("GNX_NORM_COOP", None)
            else:
                os.environ["GNX_NORM_COOP"] = before
        res["b_events"] = nb
        res["b_shift"] = x - flank
        res["b"] = {k[2:]: _stats(*v, args.warmup) for k, v in series.items() if k.startswith("b_")}
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
