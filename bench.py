#!/usr/bin/env python3
"""bench.py -- headline metric of BASELINE.json on MI355X: DP cells/s (+ aligned pairs/s) of the
affine-gap 150 bp x 10 kb batch (config C2: faChunkAlign-style reads vs one 10 kb chunk,
align.AffineGap(read, chunk, HumanChimpTwoScoreMatrix, -600, -150)).

A "step" = one pass of the hot path (forward kernel + traceback kernels, CIGARs emitted) over one batch of
`--pairs` synthetic pairs whose inputs are already resident in HBM.  One process per GPU; for N > 1 the
driver launches this file under torch.distributed.run: the 10 kb chunk is broadcast from rank 0 over
RCCL/xGMI once, every rank aligns its own shard of reads (weak scaling, no data-path collective), the
timed region is bracketed by barrier + synchronize and the max over ranks is reported.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step` and the
figures derived from the timed steps themselves (kernel_ms, roofline).  Every other measurement and check -- the device-resident rate,
the bit-exactness check against the CPU oracle, cold_plan, host_entry, the extra configurations, cpu_baseline, and under --gpus N the
ordered gather and the one_process leg -- runs only with --full (--no-cpu / --no-host / --no-extras / --verify narrow it down).
--dump-outputs DIR writes the results of the last timed step as float64 .npy files (see dump_outputs).

Objects of the line:
  roofline      algorithmic bytes (n + m + ceil(b*nm/8) + ceil(b*(n+m)/8) + 8 + 16|cigar| per pair, b = 6 bits affine /
                2 bits constant gap) / average duration of the dominant kernel's launches (HIP events on the launch stream, inside
                the library); frac = that kernel alone, frac_step = the whole step, both against the 8.0 TB/s spec peak
                (frac_vs_measured_copy_bw: against the 6.29 TB/s a copy kernel reaches)
  host_entry    SURVEY 8d's metric definition: H2D of reads + kernels + D2H of scores / CIGARs through the host-buffer entry
                point a cgo shim binds, K back-to-back calls timed like the steps; also at the top level as `value_survey_8d`.
                (`value` itself stays the device-resident rate: the bench contract wants the inputs in HBM when the timed region
                starts and rules the PCIe-inclusive rate out as `value`; VERDICT r2 asked for the 8d number in the driver's line)
  north_star_1M one gnx_align_batch_windows call with the north-star batch, 1 000 000 pairs (own roofline)
  c3            config C3: one gnx_align_batch_by_offset call, 1 048 576 reads at uniform offsets of a resident 3e9-base reference
  c5            config C5: ConstGap(20 kb, 100 kb), 10 000 x 10 000 checkerboards, 1024 pairs per launch, device-resident (own roofline)
  one_process   (--gpus N > 1, after the per-rank leg) the ONE-process flow of the C ABI on all N GPUs: gnx_init_devices(N) +
                gnx_align_batch_windows / _by_offset from rank 0 -- RCCL broadcast + gather inside the library, transport reported
  cold_plan     one step whose plans are built and uploaded afresh (the timed steps re-submit one batch: plan cache hits)
  cpu_baseline  the CPU oracle ("port" of the reference algorithm; the Go reference cannot be built here) on the host
                cores this process can really use (thread count found by a scaling probe), bounded sample of the same workload

--series long = config C5: ConstGap(20 kb ONT-style read, 100 kb window, -430) with 10 000 x 10 000 checkerboards.
"""
import argparse
import ctypes
import hashlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
HBM_COPY_GBS = 6290.0   # ... 6.29 TB/s measured copy bandwidth
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "r6_hbm_traffic.json")

# series -> (gnx mode, oracle mode, gapOpen / gapPen, gapExtend, read length, window length, direction bits per cell, default pairs)
SERIES = {
    "affine": dict(mode=0, omode=0, go=-600, ge=-150, n=150, m=10000, bits=6, pairs=100000, shared=True,
                   call="align.AffineGap", cfg="C2 faChunkAlign-style"),
    "const": dict(mode=1, omode=1, go=-430, ge=0, n=150, m=10000, bits=2, pairs=100000, shared=True,
                  call="align.ConstGap", cfg="C2 shape"),
    "local": dict(mode=3, omode=3, go=-600, ge=-150, n=150, m=10000, bits=6, pairs=100000, shared=True,
                  call="align.AffineGapLocal(target=chunk, query=read)", cfg="C2 shape"),
    "long": dict(mode=1, omode=1, go=-430, ge=0, n=20000, m=100000, bits=2, pairs=2048, shared=False,
                 call="align.ConstGap (10000 x 10000 checkerboards)", cfg="C5 long-read"),
}


def make_workload(seed, n_pairs, chunk=None, read_len=150, chunk_len=10000):
    """C2 generator, vectorised: reads sampled at uniform offsets of one chunk (0.1 % N), 1 % substitutions,
    ~0.2 %/base indel opens (one geometric(0.5)-length indel in ~26 % of the reads)."""
    rng = np.random.default_rng(seed)
    if chunk is None:
        chunk = rng.integers(0, 4, size=chunk_len).astype(np.uint8)
        chunk[rng.random(chunk_len) < 0.001] = 4
    off = rng.integers(0, chunk_len - read_len - 64, size=n_pairs)
    x = np.arange(read_len)[None, :]
    has_indel = rng.random(n_pairs) < 0.26
    pos = rng.integers(10, read_len - 10, size=n_pairs)
    ln = np.minimum(rng.geometric(0.5, size=n_pairs), 32)
    is_del = rng.random(n_pairs) < 0.5
    shift = np.where(has_indel[:, None] & (x >= pos[:, None]), np.where(is_del, ln, -ln)[:, None], 0)
    src = off[:, None] + x + shift
    reads = chunk[np.clip(src, 0, chunk_len - 1)]
    ins_mask = has_indel[:, None] & (~is_del)[:, None] & (x >= pos[:, None]) & (x < (pos + ln)[:, None])
    reads = np.where(ins_mask, rng.integers(0, 4, size=reads.shape), reads)
    sub = rng.random(reads.shape) < 0.01
    reads = np.where(sub, rng.integers(0, 4, size=reads.shape), reads).astype(np.uint8)
    return np.ascontiguousarray(reads), chunk


def make_long_workload(seed, n_pairs, n=20000, m=100000):
    """C5 generator: per pair one random 100 kb window and a 20 kb ONT-like read of a slice of it
    (per source base: 3 % deleted, 4 % substituted, 3 % preceded by a random inserted base).  Returns (reads [P, n], windows [P, m])."""
    rng = np.random.default_rng(seed)
    reads = np.zeros((n_pairs, n), dtype=np.uint8)
    wins = rng.integers(0, 4, size=(n_pairs, m), dtype=np.uint8)
    span = n + n // 8
    for p in range(n_pairs):
        off = int(rng.integers(0, m - span))
        src = wins[p, off:off + span]
        r = rng.random(span)
        keep = r >= 0.03
        base = np.where(r < 0.07, rng.integers(0, 4, size=span, dtype=np.uint8), src)
        ins = rng.random(span) < 0.03
        cnt = keep.astype(np.int64) + ins.astype(np.int64)
        out = np.repeat(base, cnt)
        start = np.cumsum(cnt) - cnt
        out[start[ins]] = rng.integers(0, 4, size=int(ins.sum()), dtype=np.uint8)
        reads[p] = out[:n]
    return reads, wins


def algorithmic_bytes(n, m, bits, pairs, total_ops):
    per_pair = n + m + (n * m * bits + 7) // 8 + ((n + m) * bits + 7) // 8 + 8
    return per_pair * pairs + 16 * total_ops


DUMP_BYTES = 60 * 1000 * 1000  # what --dump-outputs may write in all (64 MB cap, .npy headers included)


def dump_outputs(dirname, scores, ops, off, seed=0):
    """--dump-outputs: what a caller of the timed path receives from its last step -- per pair the score and its CIGAR runs -- as float64 .npy
    files: pairs (indices of the pairs written), scores, cigar_runs (runs per pair), cigar_run_length + cigar_op (the runs of those pairs,
    concatenated in pair order).  When every pair does not fit into DUMP_BYTES, the pairs of a permutation seeded by `seed` are taken in its
    order while they fit (pairs.npy is sorted), so two builds that compute the same results write the same sample."""
    off = np.asarray(off, dtype=np.int64)
    runs = np.diff(off)
    cost = 24 + 16 * runs  # pair index, score, run count + (run length, op) per run, 8 bytes each
    if int(cost.sum()) <= DUMP_BYTES:
        pick = np.arange(runs.shape[0])
    else:
        order = np.random.default_rng(seed).permutation(runs.shape[0])
        pick = np.sort(order[:int(np.searchsorted(np.cumsum(cost[order]), DUMP_BYTES, side="right"))])
    cnt = runs[pick]
    sel = ops[np.repeat(off[pick] - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))]
    os.makedirs(dirname, exist_ok=True)
    for name, arr in (("pairs", pick), ("scores", np.asarray(scores)[pick]), ("cigar_runs", cnt),
                      ("cigar_run_length", sel["run_length"]), ("cigar_op", sel["op"])):
        np.save(os.path.join(dirname, name + ".npy"), np.asarray(arr, dtype=np.float64))
    return {"dir": dirname, "pairs": int(pick.shape[0]), "of_pairs": int(runs.shape[0]), "runs": int(cnt.sum())}


def kernel_source_hash():
    """sha256 over the kernel sources: the PMC counters in profiles/ are only valid for the kernels they were taken from"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "gonomics_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def usable_cores():
    """(nominal, affinity, cgroup quota in cores or None)"""
    nominal = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = nominal
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()[:2]
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f1, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f2:
                q, per = int(f1.read()), int(f2.read())
                if q > 0:
                    quota = q / per
        except (OSError, ValueError):
            pass
    return nominal, aff, quota


def cpu_baseline(S, scores, pair_fn, n_avail, budget_s=12.0):
    """pair_fn(k) -> (alphas, betas) lists of the first k pairs.  Finds by a scaling probe on small C2-shaped samples the thread count
    beyond which the oracle stops getting faster on this box (containers cap the CPU time of the nominal cores), then times the
    sample with that many threads."""
    import oracle
    nominal, aff, quota = usable_cores()
    cap = max(1, min(aff, int(math.ceil(quota)) if quota else aff))
    last = [None]

    def run(k, threads):
        a, b = pair_fn(k)
        t0 = time.perf_counter()
        last[0] = oracle.align_batch(S["omode"], scores, S["go"], S["ge"], a, b, 10000, 10000, threads=threads)
        return time.perf_counter() - t0

    # scaling probe (always on the cheap 150 x 10 000 affine shape: a 20 kb x 100 kb pair costs 7 s per thread)
    rng = np.random.default_rng(99)
    pa = [rng.integers(0, 4, size=150).astype(np.uint8) for _ in range(4096)]
    pb = rng.integers(0, 4, size=10000).astype(np.uint8)

    def probe(threads, per_thread):
        k = min(threads * per_thread, len(pa))
        t0 = time.perf_counter()
        oracle.align_batch(0, scores, -600, -150, pa[:k], [pb] * k, 10000, 10000, threads=threads)
        return k * 150 * 10000 / (time.perf_counter() - t0)

    probe(1, 4)
    r1 = probe(1, 24)
    curve = {1: r1}
    t = 2
    while t <= cap:
        curve[t] = probe(t, max(4, 24 // (1 + t // 16)))
        t *= 2
    if cap not in curve:
        curve[cap] = probe(cap, 4)
    best = max(curve.values())
    threads = min(t for t, v in curve.items() if v >= 0.9 * best)
    # the timed sample
    per_pair_s = S["n"] * S["m"] / (curve[threads] / threads) * (2.0 if S["bits"] == 2 and S["n"] > 160 else 1.0)
    k = int(max(threads, min(n_avail, budget_s * threads / max(per_pair_s, 1e-9))))
    k = min(k, n_avail)
    dt = run(k, threads)
    cells = k * S["n"] * S["m"]
    model = ""
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"_oracle": (last[0], k), "cpu_model": model, "value": cells / dt, "unit": "DP cells/s", "cores": threads, "kind": "port",
            "pairs_per_s": k / dt, "nominal_cores": nominal, "affinity_cores": aff, "cgroup_quota_cores": quota,
            "single_thread_cells_per_s": r1,
            "thread_scaling_probe_cells_per_s": {str(t): v for t, v in sorted(curve.items())},
            "sample": "%d pairs (%dx%d, %s generator) through oracle/gnx_oracle.c or_align_batch, %d threads (the probe's knee: more threads "
                      "add < 10 %% on this box), %.1f s" % (k, S["n"], S["m"], S["cfg"].split()[0], threads, dt)}


def _sample_check(_lib, scores, mode, go, ge, got, pick, alphas_of, betas_of):
    """bit-exactness of the picked pairs against the oracle"""
    import oracle
    a = [alphas_of(int(x)) for x in pick]
    b = [betas_of(int(x)) for x in pick]
    exp = oracle.align_batch(mode, scores, go, ge, a, b, 10000, 10000, threads=min(len(a), os.cpu_count() or 1))
    sc, ops, off = got
    for k, x in enumerate(pick):
        x = int(x)
        if int(sc[x]) != int(exp[0][k]):
            return False
        g = ops[int(off[x]):int(off[x + 1])]
        e = exp[1][int(exp[2][k]):int(exp[2][k + 1])]
        if len(g) != len(e) or not np.array_equal(g["run_length"], e["run_length"]) or not np.array_equal(g["op"], e["op"]):
            return False
    return True


def _roofline_of(tm, n, m, bits, pairs, total_ops):
    launches = max(int(tm["dominant_launches"]), 1)
    avg_ms = tm["dominant_ms"] / launches
    per_launch = pairs / launches
    ab = algorithmic_bytes(n, m, bits, per_launch, total_ops / launches)
    ach = ab / (avg_ms * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
            "avg_launch_ms": avg_ms, "launches": launches, "pairs_per_launch": per_launch, "algorithmic_bytes_per_launch": ab,
            "cells_per_s_kernel": per_launch * n * m / (avg_ms * 1e-3)}


def extra_north_star(_lib, L, scores, chunk_h, dev, torch, n_pairs=1000000):
    """the north-star batch: 1 000 000 x AffineGap(150, 10 000) in ONE host-buffer call (8 pipelined sub-batches)"""
    reads, _ = make_workload(21, n_pairs, chunk_h)
    p = _lib.make_params(0, scores, -600, -150, 10000, 10000)
    h_as = np.arange(n_pairs, dtype=np.int64) * 150
    h_al = np.full(n_pairs, 150, dtype=np.int64)
    h_bs = np.zeros(n_pairs, dtype=np.int64)
    h_bl = np.full(n_pairs, chunk_h.shape[0], dtype=np.int64)
    best, tm, got, all_ms = None, None, None, []
    for _ in range(2):  # the first call sizes the pinned pools
        got = _lib.align_batch_windows(p, reads.reshape(-1), h_as, h_al, chunk_h, h_bs, h_bl)
        t = _lib.get_timing()
        all_ms.append(t["host_ms"])
        if best is None or t["host_ms"] < best:
            best, tm = t["host_ms"], t
    cells = n_pairs * 150 * chunk_h.shape[0]
    pick = np.linspace(0, n_pairs - 1, 48).astype(np.int64)
    okk = _sample_check(_lib, scores, 0, -600, -150, got, pick, lambda x: reads[x], lambda x: chunk_h)
    return {"entry": "gnx_align_batch_windows", "pairs": n_pairs, "value": cells / (best * 1e-3), "value_is": "best of 2 calls, library clock (entry to return), PCIe-inclusive",
            "unit": "DP cells/s", "pairs_per_s": n_pairs / (best * 1e-3), "ms_per_call": best, "all_calls_ms": all_ms, "kernels_ms": tm["total_ms"], "first_upload_ms": tm["stage0_ms"], "fetch_ms": tm["fetch_ms"],
            "bit_exact_sample": okk, "bit_exact_pairs_checked": int(pick.shape[0]),
            "roofline": _roofline_of(tm, 150, chunk_h.shape[0], 6, n_pairs, int(got[2][-1]))}


def extra_c3(_lib, L, scores, chunk_h, dev, torch, n_pairs=1 << 20, ref_len=3000000000, ref_seed=3):
    """config C3: reads against windows at uniform offsets of a resident 3e9-base reference generated on the device"""
    import common
    window = 10000
    reads, starts = common.c3_reads(31, n_pairs, ref_len, ref_seed, window)
    _lib.check(L.gnx_set_reference_synthetic(ref_len, ref_seed))
    try:
        p = _lib.make_params(0, scores, -600, -150, 10000, 10000)
        a_off = np.arange(n_pairs + 1, dtype=np.int64) * 150
        wl = np.full(n_pairs, window, dtype=np.int64)
        best, tm, got, all_ms = None, None, None, []
        for _ in range(2):
            got = _lib.align_batch_by_offset(p, reads.reshape(-1), a_off, starts, wl)
            t = _lib.get_timing()
            all_ms.append(t["host_ms"])
            if best is None or t["host_ms"] < best:
                best, tm = t["host_ms"], t
    finally:
        _lib.check(L.gnx_set_reference_synthetic(0, ref_seed))  # release the 0.75 GB packed reference on every context
    cells = n_pairs * 150 * window
    pick = np.linspace(0, n_pairs - 1, 48).astype(np.int64)
    okk = _sample_check(_lib, scores, 0, -600, -150, got, pick, lambda x: reads[x], lambda x: _lib.synthetic_reference_bases(int(starts[x]), window, ref_seed))
    return {"entry": "gnx_set_reference_synthetic + gnx_align_batch_by_offset", "reads": n_pairs, "reference_bases": ref_len, "value": cells / (best * 1e-3),
            "value_is": "best of 2 calls, library clock (entry to return), PCIe-inclusive", "all_calls_ms": all_ms, "unit": "DP cells/s", "reads_per_s": n_pairs / (best * 1e-3), "ms_per_call": best, "kernels_ms": tm["total_ms"],
            "bit_exact_sample": okk, "bit_exact_pairs_checked": int(pick.shape[0]),
            "roofline": _roofline_of(tm, 150, window, 6, n_pairs, int(got[2][-1]))}


def extra_c3_10m(_lib, L, scores, chunk_h, dev, torch, n_calls=10, n_pairs=1 << 20, ref_len=3000000000, ref_seed=3, n_check=10000):
    """config C3 AT ITS STATED SIZE (BASELINE.json configs[2]: 10 M 150 bp reads vs a 3 Gb reference): n_calls gnx_align_batch_by_offset
    calls of 1 Mi reads each ("batches of 1 M") = 10 485 760 reads, every batch with its own windows and reads (generated on
    the device with the binding's splitmix64 restatement), n_check pairs spread over all batches and all sub-batches against the
    oracle, every pair's CIGAR checked to consume its read and its window.  value = total cells / sum of the library's call times."""
    import common
    import oracle
    window = 10000
    _lib.check(L.gnx_set_reference_synthetic(ref_len, ref_seed))
    call_ms, kern_ms, dom_ms, dom_l, total_ops, okk, consumed = [], 0.0, 0.0, 0, 0, True, True
    per = max(1, n_check // n_calls)
    try:
        p = _lib.make_params(0, scores, -600, -150, 10000, 10000)
        a_off = np.arange(n_pairs + 1, dtype=np.int64) * 150
        wl = np.full(n_pairs, window, dtype=np.int64)
        for c in range(n_calls):
            reads, starts = common.c3_reads_torch(1000 + c, n_pairs, ref_len, ref_seed, window, 150, dev)
            got = _lib.align_batch_by_offset(p, reads.reshape(-1), a_off, starts, wl)
            t = _lib.get_timing()
            call_ms.append(t["host_ms"]); kern_ms += t["total_ms"]; dom_ms += t["dominant_ms"]; dom_l += t["dominant_launches"]
            sc, ops, off = got
            total_ops += int(off[-1])
            # every pair: the runs consume exactly the read (M + D) and the window (M + I)
            seg = np.repeat(np.arange(n_pairs), np.diff(off))
            rl = ops["run_length"]
            rows = np.bincount(seg, weights=np.where(ops["op"] != 1, rl, 0), minlength=n_pairs)
            cols = np.bincount(seg, weights=np.where(ops["op"] != 2, rl, 0), minlength=n_pairs)
            consumed = consumed and bool(np.all(rows == 150) and np.all(cols == window))
            pick = np.linspace(0, n_pairs - 1, per).astype(np.int64)
            okk = okk and _sample_check(_lib, scores, 0, -600, -150, got, pick, lambda x: reads[x],
                                        lambda x: _lib.synthetic_reference_bases(int(starts[x]), window, ref_seed))
    finally:
        _lib.check(L.gnx_set_reference_synthetic(0, ref_seed))
    n_tot = n_calls * n_pairs
    cells = n_tot * 150 * window
    tm = {"dominant_ms": dom_ms, "dominant_launches": dom_l}
    return {"entry": "gnx_set_reference_synthetic + %d x gnx_align_batch_by_offset(1 Mi reads)" % n_calls, "reads": n_tot, "reference_bases": ref_len,
            "value": cells / (sum(call_ms) * 1e-3), "value_is": "all calls, library clock (entry to return), PCIe-inclusive; read generation between the calls excluded",
            "unit": "DP cells/s", "reads_per_s": n_tot / (sum(call_ms) * 1e-3), "all_calls_ms": call_ms, "kernels_ms": kern_ms,
            "bit_exact_sample": bool(okk and consumed), "bit_exact_pairs_checked": per * n_calls, "every_pair_consumes_read_and_window": consumed,
            "roofline": _roofline_of(tm, 150, window, 6, n_tot, total_ops)}


def extra_c5(_lib, L, scores, chunk_h, dev, torch, n_pairs=1024, n=20000, m=100000):
    """config C5: ConstGap(20 kb read, 100 kb window, -430), 10 000 x 10 000 checkerboards, one launch, inputs and outputs in HBM"""
    reads, wins = make_long_workload(5, n_pairs, n, m)
    p = _lib.make_params(1, scores, -430, 0, 10000, 10000)
    d_a = torch.from_numpy(reads.reshape(-1)).to(dev)
    d_b = torch.from_numpy(wins.reshape(-1)).to(dev)
    h_as, h_bs = np.arange(n_pairs, dtype=np.int64) * n, np.arange(n_pairs, dtype=np.int64) * m
    h_al, h_bl = np.full(n_pairs, n, dtype=np.int64), np.full(n_pairs, m, dtype=np.int64)
    d_as, d_bs, d_al, d_bl = (torch.from_numpy(x).to(dev) for x in (h_as, h_bs, h_al, h_bl))
    d_score = torch.zeros(n_pairs, dtype=torch.int64, device=dev)
    d_off = torch.zeros(n_pairs + 1, dtype=torch.int64, device=dev)
    cap = 31000 * n_pairs
    d_ops = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
    tot = ctypes.c_int64()
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        _lib.check(L.gnx_align_batch_device(ctypes.byref(p), n_pairs, d_a.data_ptr(), d_as.data_ptr(), d_al.data_ptr(), d_b.data_ptr(), d_bs.data_ptr(), d_bl.data_ptr(),
                                            h_al.ctypes.data, h_bl.ctypes.data, d_score.data_ptr(), d_ops.data_ptr(), cap, d_off.data_ptr(), ctypes.byref(tot), ctypes.c_void_p(stream)))
    try:  # sizing call: a 20 kb read against 100 kb has tens of thousands of CIGAR runs
        step()
    except _lib.GnxError as e:
        if e.code != _lib.GNX_ECAPACITY:
            raise
        cap = int(tot.value * 1.05) + 1024
        d_ops = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tm = _lib.get_timing()
    sc = d_score.cpu().numpy()
    off = d_off.cpu().numpy()
    ops = d_ops[:int(off[-1]) * 16].cpu().numpy().view(_lib.CIGAR_DTYPE)
    pick = np.linspace(0, n_pairs - 1, 8).astype(np.int64)  # (a 20 kb x 100 kb pair costs the oracle ~7 s on one thread: 8 pairs on 8 threads)
    okk = _sample_check(_lib, scores, 1, -430, 0, (sc, ops, off), pick, lambda x: reads[x], lambda x: wins[x])
    cells = n_pairs * n * m
    return {"entry": "gnx_align_batch_device (GNX_CONST_GAP)", "pairs": n_pairs, "value": cells / dt, "unit": "DP cells/s", "ms_per_step": dt * 1e3,
            "path": {0: "general_path", 1: "fast_path", 2: "const_long", 3: "latency_geometry", 4: "int64_fallback", 5: "row_panels", 6: "const_long_w64"}[tm["fast_path"]], "bit_exact_sample": okk, "bit_exact_pairs_checked": int(pick.shape[0]),
            "kernel_ms": {"sweep": tm["dominant_ms"], "walk_and_rest": tm["traceback_ms"]},
            "roofline": _roofline_of(tm, n, m, 2, n_pairs, int(off[-1])),
            # the BINDING ceiling of the constant-gap sweep: VALU issue.  The floor of the recurrence is two instructions per cell
            # (add_sdwa, max3 -- both half rate: 1.84 ns per wave-instruction slot and SIMD at >= 2 waves, profiles/r3_valu_ubench4.txt); a 20 kb read is
            # 125 strips of 160 rows = 10 rows in each of 16 lanes, four pairs share a wave
            "roofline_valu": _c5_valu_floor(tm, n, m, n_pairs, torch.cuda.get_device_properties(dev).multi_processor_count)}


def _c5_valu_floor(tm, n, m, n_pairs, n_cu):
    strips = -(-n // 160)
    slots = n_pairs * strips * (m + 15) * 10 * 2 / 4.0  # wave-instruction slots of the floor: (steps of a strip) x 10 rows x 2 instructions, 4 pairs per wave
    floor_ms = slots * 1.84e-9 / (4 * n_cu) * 1e3
    return {"bound": "valu", "floor_ms": floor_ms, "frac_of_floor": floor_ms / tm["dominant_ms"],
            "floor_model": "2 instructions per cell (add_sdwa, max3) x 1.84 ns per wave-instruction slot and SIMD (measured issue rate of half-rate VALU instructions at >= 2 waves per "
                           "SIMD, profiles/r3_valu_ubench4.txt) / (4 SIMDs x %d CUs); the kernel's own block of 16 steps is 1 DPP move + 10 x (add, max3) + ring address per step "
                           "(const_long_wg.hip.h): ~2.3 instructions per cell" % n_cu}


def extra_gsw(_lib, L, scores, chunk_h, dev, torch, n_reads=20000, n_check=48):
    """"next" row N2, the graph aligner's read path (cmd/gsw): GraphSmithWatermanToGiraf for a batch of reads as ONE C-ABI call
    (gnx_gsw_graph_create / gnx_gsw_map_reads: seed search and extension DPs on the device, the per-read driver on the library's pool of
    host threads).  4 x 200 kb graph, seedLen 32 / step 32, 150-base reads with 2 % substitutions and 1 % indels, both strands.  Not the
    headline metric; a sample is compared with the sequential restatement tests/pyref_gsw.py (CPU oracle DPs) after the timing."""
    import common
    import pyref_gsw as ref
    from gonomics_amd import genomeGraph as gg
    rng = np.random.default_rng(9)
    seed_len, step = 32, 32
    seqs = [rng.integers(0, 4, size=200000).astype(np.uint8) for _ in range(4)]
    reads = []
    for _ in range(n_reads):
        k = int(rng.integers(0, 4)); o = int(rng.integers(0, 200000 - 170))
        r = common.mutate(rng, seqs[k][o:o + 170], 0.02, 0.01)[:150]
        reads.append(r if rng.random() < 0.5 else (3 - r[::-1]).astype(np.uint8))
    cat = (np.concatenate(reads), np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.int64))
    t0 = time.perf_counter()
    h = _lib.GswGraph(seqs, [], seed_len, step)
    t_graph = time.perf_counter() - t0
    best = None
    for _ in range(4):  # (the first call uploads the index and starts the workers)
        t0 = time.perf_counter()
        gir, nodes, cig = h.map_reads(cat, scores, -600)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    h.close()
    rnodes = ref.make_graph(seqs, [])
    full = ref.index_genome(rnodes, seed_len, step)
    okk = True
    pick = np.linspace(0, n_reads - 1, n_check).astype(np.int64)
    for x in pick:
        r2 = ref.make_read(reads[int(x)])
        exp = ref.giraf_key(ref.read_to_giraf(rnodes, r2, ref.seed_map(full, rnodes, r2, seed_len), scores))
        g = gir[int(x)]
        got_c = None if not g["has_cigar"] else tuple((int(a), int(b)) for a, b in zip(cig["run_length"][int(g["cigar_off"]):int(g["cigar_off"] + g["n_cigar"])], cig["op"][int(g["cigar_off"]):int(g["cigar_off"] + g["n_cigar"])]))
        got = (int(g["q_start"]), int(g["q_end"]), bool(g["pos_strand"]), int(g["t_start"]), tuple(int(v) for v in nodes[int(g["node_off"]):int(g["node_off"] + g["n_nodes"])]), int(g["t_end"]), got_c, int(g["aln_score"]))
        okk = okk and got == tuple(exp[:8])
    return {"entry": "gnx_gsw_map_reads (one call per batch of reads)", "reads": n_reads, "value": n_reads / best, "unit": "reads/s (fastest of 4 calls)", "ms_per_call": best * 1e3,
            "mapped": int((gir["aln_score"] > 0).sum()), "graph_and_index_s": t_graph, "bit_exact_sample": bool(okk), "reads_checked": int(n_check),
            "checked_against": "tests/pyref_gsw.py (sequential restatement of toGiraf.go:17-72 with the oracle's DPs)"}


def extra_n1(_lib, L, scores, chunk_h, dev, torch):
    """N1 on the workload cmd/faChunkAlign really runs: a whole align.AllSeqAffineChunk -- 8 sequences x 30 kb, chunk 3,
    gapOpen -300, gapExtend -40, multi-fasta in / multi-fasta out through gonomics_amd.cmds.faChunkAlign -- with the fill kernel's roofline
    (6 bits per chunk cell) and the CPU oracle on first-round pairs beside it (tools/bench_n1_cmd.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_n1_cmd
    cold = bench_n1_cmd.run(8, 30000, 3, cpu_pairs=0)          # first use: 11 GB of score matrices and direction words are allocated
    out = bench_n1_cmd.run(8, 30000, 3, cpu_pairs=min(4, os.cpu_count() or 1))
    out["command_s_first_use"] = cold["command_s"]
    pr = out.pop("per_round")
    out["per_round_ms"] = [{"pairs": r["pairs"], "call": round(r["call_s"] * 1e3, 2), "fill": round(r["fill_ms"], 2), "traceback": round(r["traceback_ms"], 2), "path": r["path"]} for r in pr]
    return out


def long_pair_roofline(d, geo=None, pmc=None):
    """HBM roofline of ONE long pair on the 64-lane snapshot kernels with the bytes of SURVEY 8d, like every other leg: n + m input bases +
    ceil(b n m / 8) direction bits (b = 6 AffineGap, 2 ConstGap) + ceil(b (n + m) / 8) read along the path + 8 (score) + 16 per CIGAR run -- `frac` over the sweep
    kernel's time (the dominant kernel), `frac_call` over the whole call.  `traffic_model`: the bytes THIS design moves instead of a direction matrix -- the bottom
    row of every strip but the last, written and read once (AffineGap 8 B per column: {dn, h}; ConstGap 4 B), + a snapshot of the wavefront per strip every K steps
    ((2 RW + 2 -> multiple of 4) dwords x 64 lanes; geo = (rows per lane, K) of the call, gnx_debug_counter(5 / 6)); `traffic`: the PMC bytes per launch when the
    committed counters belong to these kernel sources.  The binding ceiling is the VALU issue of the pair's strips (one wave each), not memory."""
    affine = d["fn"].startswith("AffineGap")
    bits = 6 if affine else 2
    n, m = d["n"], d["m"]
    rw, ck = geo if geo else (10, 512 if affine else 224)
    strips = -(-n // (64 * rw))
    rows = (8 if affine else 4) * (m + 1) * max(strips - 1, 0) * 2
    snaps = ((m + 63) // ck) * strips * 64 * (((2 * rw + 2 + 3) & ~3) if affine else ((rw + 1 + 3) & ~3)) * 4
    alg = n + m + -(-bits * n * m // 8) + -(-bits * (n + m) // 8) + 8 + 16 * d["runs"]
    secs = d["sweep_ms"] * 1e-3
    ach = alg / secs / 1e9
    return {"bound": "hbm", "achieved": ach, "peak": 8000.0, "unit": "GB/s", "frac": ach / 8000.0, "frac_call": alg / d["call_s"] / 8e12, "algorithmic_bytes_per_launch": alg,
            "bytes_model": "SURVEY 8d: n + m + ceil(%d n m / 8) + ceil(%d (n + m) / 8) + 8 + 16 |cigar|" % (bits, bits),
            "traffic_model": {"bytes_per_launch": rows + snaps, "GB_per_s": (rows + snaps) / secs / 1e9, "rows_per_lane": rw, "snapshot_steps": ck,
                              "what": "bottom rows of the strips written + read once, wavefront snapshots written (this design keeps no direction matrix)"},
            "traffic": pmc, "cells_per_s_kernel": d["cells"] / secs, "waves": strips,
            "note": "binding ceiling: VALU issue of the pair's strips (one wave each on 1 024 SIMDs), see DESIGN 4.13"}


def extra_long_pairs(_lib, L, scores, chunk_h, dev, torch):
    """ONE long pair per call -- what cmd/cigarToBed (cigarToBed.go:86) and cmd/globalAlignment (globalAlignment.go:84) hand to align.AffineGap / ConstGap: the 64-lane
    snapshot kernels + walk farm.  Every pair that has a CPU-oracle digest in tests/golden/long_pairs.json must equal it (ConstGap 150 kb x 180 kb,
    AffineGap 340 kb x 340 kb, the quirk-Q1 pair 300 kb x 298 kb, AffineGap 1 Mb x 1 Mb: 185 s .. 2 h of one core each); without one, the CIGAR must consume both
    sequences and re-score (int64) to within 600 x (quirk-Q1 restarts that changed the walk's state) below the score -- and to the score itself when there was none."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import long_pairs
    rows = list(long_pairs.gpu_rows(["const_150k", "affine_340k", "affine_q1_300k", "affine_1M"], reps=2))
    keep = ("case", "fn", "n", "m", "cells", "call_s", "first_call_s", "sweep_ms", "walk_ms", "cells_per_s_call", "workspace_bytes", "route", "score", "runs", "consumes_n_m",
            "rescored_equals_score", "rescored_minus_score", "q1_restarts", "q1_restarts_changed", "equals_oracle", "rows_per_lane", "snapshot_steps")
    ok = all(long_pairs.row_ok(r) for r in rows)
    pairs = [{k: r[k] for k in keep if k in r} for r in rows]
    pmc = None
    try:  # HBM bytes per launch of the 1 Mb sweep from the committed counter passes, if they belong to these kernel sources
        with open(os.path.join(ROOT, "profiles", "r6_pmc_long_pair.json")) as fh:
            pj = json.load(fh)
        pmc = pj if pj.get("kernel_source_hash") == kernel_source_hash() else {"stale": "collected from other kernel sources (commit %s)" % pj.get("commit")}
    except (OSError, ValueError):
        pass
    for d in pairs:
        d["sweep_roofline"] = long_pair_roofline(d, (d["rows_per_lane"], d["snapshot_steps"]) if "rows_per_lane" in d else None, (pmc or {}).get(d["case"]) if pmc and "stale" not in pmc else pmc)
    return {"entry": "gnx_align_batch (one pair per call, host buffers)", "pairs": pairs, "bit_exact_sample": bool(ok),
            "checked_against": "sha256 of the CPU oracle's CIGAR where tests/golden/long_pairs.json holds one; else consumed lengths + int64 re-score bounded by the quirk-Q1 restarts the walk reports"}


def one_process_flow(_lib, L, world, params, reads_h, chunk_h, n_pairs, same, steps, share_gpu=False):
    """SURVEY 8e, second form: ONE host process, one context per GPU behind the C ABI (what a Go program gets).  Rank 0 runs it on
    all `world` GPUs after the other ranks have released theirs: `world` x n_pairs reads against the shared chunk (broadcast over
    RCCL inside the call), then the same reads against the chunk as resident reference; compared with the one-GPU result."""
    reads = np.concatenate([reads_h] + [make_workload(2 + 1000 * r, n_pairs, chunk_h)[0] for r in range(1, world)])
    n = reads.shape[0]
    h_as = np.arange(n, dtype=np.int64) * 150
    h_al = np.full(n, 150, dtype=np.int64)
    h_bs = np.zeros(n, dtype=np.int64)
    h_bl = np.full(n, chunk_h.shape[0], dtype=np.int64)
    _lib.check(L.gnx_init(0, 0))
    ref_res = _lib.align_batch_windows(params, reads.reshape(-1), h_as, h_al, chunk_h, h_bs, h_bl)  # one context, one GPU
    one_ms = _lib.get_timing()["host_ms"]
    L.gnx_shutdown()
    if share_gpu:  # flow check on a 1-GPU box: `world` contexts on device 0, the exchange by peer copies (RCCL wants distinct devices)
        os.environ["GNX_RCCL"] = "0"
    nd = _lib.init_devices([0] * world if share_gpu else list(range(world)), 0)
    out = {"contexts": nd, "pairs": n}
    calls = []
    got = None
    for _ in range(1 + max(steps, 2)):
        got = _lib.align_batch_windows(params, reads.reshape(-1), h_as, h_al, chunk_h, h_bs, h_bl)
        calls.append(_lib.get_timing())
    tm = min(calls[1:], key=lambda t: t["host_ms"])
    cells = n * 150 * chunk_h.shape[0]
    out["windows"] = {"value": cells / (tm["host_ms"] * 1e-3), "unit": "DP cells/s", "ms_per_call": tm["host_ms"], "all_calls_ms": [t["host_ms"] for t in calls],
                      "kernels_ms_slowest_context": tm["total_ms"], "gather_ms": tm["gather_ms"], "bcast_ms": tm["bcast_ms"], "fetch_ms": tm["fetch_ms"],
                      "transport": {0: "none", 1: "rccl", 2: "peer copies", 3: "peer copies after a RCCL failure"}[tm["transport"]],
                      "rccl_ranks": nd if tm["transport"] == 1 else 0, "cells_per_gpu": cells // nd, "one_gpu_ms": one_ms,
                      "speedup_vs_one_gpu": one_ms / tm["host_ms"], "equals_one_gpu": same(got, ref_res)}
    _lib.set_reference(chunk_h)
    a_off = np.arange(n + 1, dtype=np.int64) * 150
    got2 = _lib.align_batch_by_offset(params, reads.reshape(-1), a_off, h_bs, h_bl)
    got2 = _lib.align_batch_by_offset(params, reads.reshape(-1), a_off, h_bs, h_bl)
    t2 = _lib.get_timing()
    out["by_offset"] = {"value": cells / (t2["host_ms"] * 1e-3), "unit": "DP cells/s", "ms_per_call": t2["host_ms"], "gather_ms": t2["gather_ms"],
                        "transport": t2["transport"], "equals_one_gpu": same(got2, ref_res)}
    out["bit_exact_sample"] = bool(out["windows"]["equals_one_gpu"] and out["by_offset"]["equals_one_gpu"])
    out["last_error_text"] = (L.gnx_last_error() or b"").decode("utf-8", "replace")  # non-empty after a RCCL failure that was survived
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=0, help="pairs per GPU per step (default: 100 k for the C2 series, 2048 for --series long)")
    ap.add_argument("--ws-gb", type=float, default=150.0, help="workspace limit per GPU")
    ap.add_argument("--full", action="store_true", help="after the headline, every other leg and check: device-resident rate, oracle check, cold_plan, "
                                                         "host_entry, extras, cpu_baseline; under --gpus N the ordered gather and one_process")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the results of the last timed step to DIR/<name>.npy (rank 0's pairs)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--no-host", action="store_true", help="with --full: skip the host_entry and cold_plan legs")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the north_star_1M / c3 / c5 / n1 / gsw_reads / long_pairs sub-objects (and one_process under --gpus N)")
    ap.add_argument("--verify", type=int, default=-1, help="pairs checked bit-exactly against the oracle after timing (default: 32 with --full, 2 for --series long; 0 without)")
    ap.add_argument("--dist-backend", default="nccl", help="debug: 'gloo' lets several ranks share one GPU (with --share-gpu)")
    ap.add_argument("--share-gpu", action="store_true", help="debug: every rank uses cuda:0 (flow check of the N>1 path on a 1-GPU box)")
    ap.add_argument("--one-process", action="store_true", help="run the one_process leg even with --share-gpu / --no-extras (contexts on cuda:0, peer copies)")
    ap.add_argument("--series", default="affine", choices=sorted(SERIES),
                    help="affine = the headline AffineGap(read, chunk); const = ConstGap(read, chunk, -430); "
                         "local = AffineGapLocal(target=chunk, query=read) (SURVEY 8d second series); long = config C5")
    args = ap.parse_args()
    S = SERIES[args.series]
    READ_LEN, CHUNK_LEN = S["n"], S["m"]

    import torch
    import torch.distributed as dist
    from gonomics_amd import _lib, align, shard

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        sys.exit("launch with: python -m torch.distributed.run --nnodes=1 --nproc-per-node %d bench.py --gpus %d ..." % (args.gpus, args.gpus))
    dev_index = 0 if args.share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI
        else:
            dist.init_process_group(args.dist_backend)
    L = _lib.lib()
    ws_gb = args.ws_gb / (world if args.share_gpu else 1)
    _lib.check(L.gnx_init(dev_index, int(ws_gb * (1 << 30))))

    n_pairs = args.pairs or S["pairs"]
    n_verify = args.verify if args.verify >= 0 else (0 if not args.full else 2 if args.series == "long" else 32)
    checked = args.full or n_verify > 0  # bit_exact_sample is null when nothing was checked
    scores = align.HumanChimpTwoScoreMatrix
    if S["shared"]:
        # rank 0 owns the chunk; everyone gets it by broadcast (RCCL over xGMI when world > 1)
        if rank == 0:
            reads0, chunk_h = make_workload(2, n_pairs)
        else:
            chunk_h = np.zeros(CHUNK_LEN, dtype=np.uint8)
        d_chunk = torch.from_numpy(chunk_h).to(dev)
        if world > 1:
            shard.broadcast_reference(d_chunk, src=0)  # RCCL broadcast over xGMI
            chunk_h = d_chunk.cpu().numpy()
        reads_h = reads0 if rank == 0 else make_workload(2 + 1000 * rank, n_pairs, chunk_h)[0]
        h_bs = np.zeros(n_pairs, dtype=np.int64)
        beta_h = chunk_h
    else:
        # C5: every pair has its own window (independent pairs; nothing to broadcast).  ONE shared list of world x n_pairs pairs, cut into contiguous blocks
        # of equal DP cells (shard.partition_by_cells); block r of the list is generated from seed 5 + 1000 r, so a rank builds only its own
        shared_alen = np.full(n_pairs * world, READ_LEN, dtype=np.int64)
        shared_blen = np.full(n_pairs * world, CHUNK_LEN, dtype=np.int64)
        bounds = shard.partition_by_cells(shared_alen, shared_blen, world) if world > 1 else np.asarray([0, n_pairs])
        assert int(bounds[rank]) == rank * n_pairs and int(bounds[rank + 1]) == (rank + 1) * n_pairs, bounds  # (equal pairs: equal counts)
        reads_h, wins_h = make_long_workload(5 + 1000 * rank, n_pairs, READ_LEN, CHUNK_LEN)
        d_chunk = torch.from_numpy(wins_h.reshape(-1)).to(dev)
        h_bs = np.arange(n_pairs, dtype=np.int64) * CHUNK_LEN
        beta_h = wins_h.reshape(-1)
    d_reads = torch.from_numpy(reads_h.reshape(-1)).to(dev)
    h_alen = np.full(n_pairs, READ_LEN, dtype=np.int64)
    h_blen = np.full(n_pairs, CHUNK_LEN, dtype=np.int64)
    h_as = np.arange(n_pairs, dtype=np.int64) * READ_LEN
    d_as = torch.from_numpy(h_as).to(dev)
    d_al = torch.from_numpy(h_alen).to(dev)
    d_bs = torch.from_numpy(h_bs).to(dev)
    d_bl = torch.from_numpy(h_blen).to(dev)
    d_score = torch.zeros(n_pairs, dtype=torch.int64, device=dev)
    d_off = torch.zeros(n_pairs + 1, dtype=torch.int64, device=dev)
    cap = 48 * n_pairs
    d_ops = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
    gmode, omode, go, ge = S["mode"], S["omode"], S["go"], S["ge"]
    params = _lib.make_params(gmode, scores, go, ge, 10000, 10000)
    total_ops = ctypes.c_int64()
    stream = torch.cuda.current_stream().cuda_stream
    swap = args.series == "local"  # AffineGapLocal(target=chunk, query=read): alpha is the chunk

    def step(np_=None):
        k = n_pairs if np_ is None else np_
        if swap:
            _lib.check(L.gnx_align_batch_device(ctypes.byref(params), k, d_chunk.data_ptr(), d_bs.data_ptr(), d_bl.data_ptr(),
                                                d_reads.data_ptr(), d_as.data_ptr(), d_al.data_ptr(),
                                                h_blen.ctypes.data, h_alen.ctypes.data,
                                                d_score.data_ptr(), d_ops.data_ptr(), cap, d_off.data_ptr(),
                                                ctypes.byref(total_ops), ctypes.c_void_p(stream)))
            return
        _lib.check(L.gnx_align_batch_device(ctypes.byref(params), k, d_reads.data_ptr(), d_as.data_ptr(), d_al.data_ptr(),
                                            d_chunk.data_ptr(), d_bs.data_ptr(), d_bl.data_ptr(),
                                            h_alen.ctypes.data, h_blen.ctypes.data,
                                            d_score.data_ptr(), d_ops.data_ptr(), cap, d_off.data_ptr(),
                                            ctypes.byref(total_ops), ctypes.c_void_p(stream)))

    # `value`: SURVEY 8d defines the metric over "H2D of reads + kernels + D2H of scores / CIGARs", so the timed
    # steps of the C2-shaped series are calls of the HOST-buffer entry point a cgo shim binds (gnx_align_batch_windows: pageable numpy
    # arrays in, pinned result arrays out); the device-resident rate of the same batch is measured after it and reported as
    # `value_device_resident`.  --series long (C5) stays device-resident (its inputs are per-pair windows, 0.25 GB per 2048 pairs).
    host_timed = bool(S["shared"])
    a_buf_h, b_buf_h = np.ascontiguousarray(reads_h.reshape(-1)), np.ascontiguousarray(beta_h)
    h_scores = np.zeros(n_pairs, dtype=np.int64)

    def host_step():
        if swap:
            return _lib.align_batch_windows_raw(params, b_buf_h, h_bs, h_blen, a_buf_h, h_as, h_alen, h_scores)
        return _lib.align_batch_windows_raw(params, a_buf_h, h_as, h_alen, b_buf_h, h_bs, h_blen, h_scores)

    def size_device_buffers():
        nonlocal cap, d_ops
        try:  # one untimed sizing call: const-gap CIGARs have hundreds (C5: tens of thousands) of runs per pair
            step()
        except _lib.GnxError as e:
            if e.code != _lib.GNX_ECAPACITY:
                raise
            cap = int(total_ops.value * 1.05) + 1024
            d_ops = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)

    fill_ms, tb_ms, launches, host_ms = [], [], 0, []
    dom_ms, dom_launches, fast_path = 0.0, 0, 0
    got_main = None
    if host_timed:
        for _ in range(args.warmup):
            host_step().free()
        last = None
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if last is not None:
                last.free()
            last = host_step()
            tm = _lib.get_timing()
            fill_ms.append(tm["fill_ms"]); tb_ms.append(tm["traceback_ms"]); launches += tm["n_launches"]; host_ms.append(tm["host_ms"])
            dom_ms += tm["dominant_ms"]; dom_launches += tm["dominant_launches"]; fast_path = tm["fast_path"]
        torch.cuda.synchronize()
        dt_own = time.perf_counter() - t0  # this rank's own K steps, before it waits for the others
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        got_main = last.copy()
        last.free()
        step_total_ops = int(got_main[2][-1])
        dt_dev = None
        if args.full:
            # the same batch with inputs and outputs resident in HBM (gnx_align_batch_device), timed the same way, per rank
            size_device_buffers()
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dev_dom_ms, dev_dom_launches = 0.0, 0
            for _ in range(args.steps):
                step()
                tmd = _lib.get_timing()
                dev_dom_ms += tmd["dominant_ms"]; dev_dom_launches += tmd["dominant_launches"]
            torch.cuda.synchronize()
            dt_dev = time.perf_counter() - t1
    else:
        size_device_buffers()
        for _ in range(args.warmup):
            step()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
            tm = _lib.get_timing()
            fill_ms.append(tm["fill_ms"]); tb_ms.append(tm["traceback_ms"]); launches += tm["n_launches"]
            dom_ms += tm["dominant_ms"]; dom_launches += tm["dominant_launches"]; fast_path = tm["fast_path"]
        torch.cuda.synchronize()
        dt_own = time.perf_counter() - t0
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        dt_dev = dt
        step_total_ops = total_ops.value
    rank_ms = [dt_own / args.steps * 1e3]
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # every rank's own time per step (before the closing barrier): a straggler rank shows in the first SCALE line
        mine = torch.tensor([dt_own / args.steps * 1e3], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        rank_ms = [float(x.item()) for x in every]

    def fetch(k):
        if got_main is not None and k <= n_pairs:  # the results of the last timed (host-entry) step
            o = got_main[2]
            return got_main[0][:k], got_main[1][:int(o[k])], o[:k + 1]
        return fetch_device(k)

    def fetch_device(k):
        sc = d_score[:k].cpu().numpy()
        off = d_off[:k + 1].cpu().numpy()
        ops = d_ops[:int(off[-1]) * 16].cpu().numpy().view(_lib.CIGAR_DTYPE)
        return sc, ops, off

    def pair_lists(k):
        a = [reads_h[x] for x in range(k)]
        b = [beta_h[h_bs[x]:h_bs[x] + CHUNK_LEN] for x in range(k)]
        return (b, a) if swap else (a, b)

    def same(got, exp):
        return bool(np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[2]) and np.array_equal(got[1]["run_length"], exp[1]["run_length"])
                    and np.array_equal(got[1]["op"], exp[1]["op"]))

    # ---- after the timed region: the outputs, verification + the other legs (rank 0) ----
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, *fetch(n_pairs))
    ok = True
    gathered_pairs = n_pairs if world == 1 else None  # (N > 1: set by the gather, which runs with --full)
    gather_order_ok = None
    if n_verify > 0:
        import oracle
        k = min(n_verify, n_pairs)
        a, b = pair_lists(k)
        ok = same(fetch(k), oracle.align_batch(omode, scores, go, ge, a, b, 10000, 10000, threads=min(k, os.cpu_count() or 1)))
    if world > 1:
        f = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(f, op=dist.ReduceOp.MIN)
        ok = bool(f.item())
    if world > 1 and args.full:
        # final gather of scores / CIGAR offsets / CIGAR blob on rank 0, in input order (outside the timed region)
        n_ops_local = int(d_off[n_pairs].item())
        gathered = shard.gather_results(d_score, d_ops[: n_ops_local * 16], d_off, dst=0)
        # the gathered arrays are in INPUT order (rank r's block at pairs [r n, (r + 1) n)): every rank reports its block's first / last score, run counts and
        # a sum of its run lengths; rank 0 finds them at those places of what it gathered
        ops_local = d_ops[: n_ops_local * 16].view(torch.int64).view(-1, 2)[:, 0] if n_ops_local else torch.zeros(0, dtype=torch.int64, device=dev)
        sig = torch.stack([d_score[0], d_score[n_pairs - 1], d_off[1] - d_off[0], d_off[n_pairs] - d_off[n_pairs - 1], ops_local.sum()]).to(torch.int64)
        sigs = [torch.zeros_like(sig) for _ in range(world)]
        dist.all_gather(sigs, sig)
        if rank == 0:
            gathered_pairs = int(gathered[0].numel())
            ok = ok and gathered_pairs == n_pairs * world and int(gathered[2][-1].item()) * 16 == gathered[1].numel()
            gather_order_ok = gathered_pairs == n_pairs * world
            g_sc, g_ops, g_off = gathered[0], gathered[1].view(torch.int64).view(-1, 2)[:, 0], gathered[2]
            for r in range(world if gather_order_ok else 0):
                b0, b1 = r * n_pairs, (r + 1) * n_pairs
                mine = torch.stack([g_sc[b0], g_sc[b1 - 1], g_off[b0 + 1] - g_off[b0], g_off[b1] - g_off[b1 - 1], g_ops[int(g_off[b0].item()):int(g_off[b1].item())].sum()])
                gather_order_ok = gather_order_ok and bool(torch.equal(mine, sigs[r]))
            ok = ok and gather_order_ok
    if rank == 0:
        cells_per_step = n_pairs * READ_LEN * CHUNK_LEN * world
        value = cells_per_step * args.steps / dt
        ms_per_step = dt / args.steps * 1e3
        fill_avg_ms = dom_ms / max(dom_launches, 1)  # average duration of the dominant kernel's launches (HIP events)
        pairs_per_launch = n_pairs * args.steps / max(dom_launches, 1)
        abytes = algorithmic_bytes(READ_LEN, CHUNK_LEN, S["bits"], pairs_per_launch, step_total_ops * pairs_per_launch / n_pairs)
        abytes_step = algorithmic_bytes(READ_LEN, CHUNK_LEN, S["bits"], n_pairs, step_total_ops)
        achieved = abytes / (fill_avg_ms * 1e-3) / 1e9
        achieved_step = abytes_step * world / (ms_per_step * 1e-3) / 1e9 / world  # per GPU
        path = {0: "general_path", 1: "fast_path", 2: "const_long", 3: "latency_geometry", 4: "int64_fallback", 5: "row_panels", 6: "const_long_w64"}[fast_path]
        kernel = {0: "fill_affine_kernel (full direction matrix)" if S["bits"] == 6 else "fill_const_kernel (full direction matrix)",
                  1: "fp_sweep_kernel<%d, %s> (fast-path forward sweep)" % (19 if READ_LEN <= 152 else 20, "true" if swap else "false"),
                  2: "cl_sweep_wg_kernel<4> (score-only constant-gap sweep with wavefront snapshots, four strips per workgroup handing rows over through LDS)",
                  3: "lat_fill_kernel (one pair per wave, 64 lanes x 2 rows, full direction matrix)", 4: "lat_wide_kernel (int64 keys)",
                  5: "al64_sweep_kernel / cl64_sweep_kernel in row panels (run_device_mega)", 6: "al64_sweep_kernel / cl64_sweep_kernel (64 lanes per pair, score only, snapshots)"}.get(fast_path, path)
        # HBM bytes per launch of the dominant kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE), valid
        # only for the kernel sources they were taken from
        traffic, traffic_note, pmc = None, None, None
        try:
            with open(TRAFFIC_FILE) as fh:
                tj = json.load(fh)
            if tj.get("kernel_source_hash") != kernel_source_hash():
                traffic_note = "stale: %s was collected at commit %s from other kernel sources" % (os.path.basename(TRAFFIC_FILE), tj.get("commit"))
            else:
                pmc = tj.get(args.series, {}).get(path)
                if pmc:
                    traffic = pmc["hbm_bytes_per_pair"] * pairs_per_launch
                    traffic_note = "bytes per launch (PMC, %s, commit %s)" % (os.path.basename(TRAFFIC_FILE), tj.get("commit"))
        except (OSError, KeyError, ValueError):
            traffic_note = "no PMC file"
        out = {
            "metric": "DP cells/sec + aligned pairs/sec, affine-gap 150bp x 10kb batch" if args.series == "affine"
                      else "DP cells/sec, series=%s (not the headline metric)" % args.series,
            "value": value, "unit": "DP cells/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "int32", "data": "synthetic",
            "config": {"workload": "%s: %d x (%d bp read vs %s) per GPU, %s, HumanChimpTwoScoreMatrix, %s, score + full CIGAR"
                                   % (S["cfg"], n_pairs, READ_LEN, "one 10 kb chunk" if S["shared"] else "its own %d bp window" % CHUNK_LEN, S["call"],
                                      "gapPen %d" % go if S["bits"] == 2 else "gapOpen %d, gapExtend %d" % (go, ge)),
                       "pairs_per_gpu": n_pairs, "read_len": READ_LEN, "chunk_len": CHUNK_LEN, "parallelism": "pairs sharded x%d" % world,
                       "plan_cache": "the timed steps re-submit one batch, so the fast path's per-pair plans are reused on the device (see cold_plan)"},
            "pairs_per_s": n_pairs * world * args.steps / dt,
            "per_rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms), "all": rank_ms,
                                     "note": "each rank's own K steps / K, before the closing barrier (ms_per_step is the max-over-ranks clock around both barriers)"},
            "gathered_pairs": gathered_pairs, "gather_order_ok": (gather_order_ok if world > 1 else None),
            "value_definition": ("SURVEY 8d: sum n*m over pairs / wall time of K calls of the host-buffer entry point (H2D of reads, windows and offset tables + plans + "
                                 "kernels + D2H of scores / offsets / CIGAR runs into pinned host arrays); the chunk upload is part of every call")
                                if host_timed else "inputs and outputs resident in HBM (gnx_align_batch_device)",
            "bit_exact_sample": ok if checked else None, "bit_exact_pairs_checked": int(min(n_verify, n_pairs)),
            "kernel_ms": {"all_fill_kernels_per_step": float(np.mean(fill_ms)), "traceback_and_rest_per_step": float(np.mean(tb_ms)),
                          "dominant_kernel_per_step": dom_ms / args.steps, "path": path, "launches_per_step": launches / args.steps},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_note": traffic_note,
                         "kernel": kernel, "avg_launch_ms": fill_avg_ms,
                         "algorithmic_bytes_per_launch": abytes, "direction_bits_per_cell": S["bits"],
                         "cells_per_s_kernel": pairs_per_launch * READ_LEN * CHUNK_LEN / (fill_avg_ms * 1e-3),
                         "frac_vs_measured_copy_bw": achieved / HBM_COPY_GBS,
                         "achieved_step": achieved_step, "frac_step": achieved_step / HBM_PEAK_GBS,
                         "frac_step_vs_measured_copy_bw": achieved_step / HBM_COPY_GBS},
        }
        if dt_dev is not None:
            out.update({"value_device_resident": cells_per_step / world * args.steps / dt_dev, "ms_per_step_device_resident": dt_dev / args.steps * 1e3,
                        "value_device_resident_note": "rank 0's GPU alone, same batch through gnx_align_batch_device, K steps timed the same way"})
        if dumped:
            out["outputs_dumped"] = dumped
        if pmc and pmc.get("valu_insts_per_pair"):
            # second ceiling: VALU issue, 256 CU x 4 SIMD x 32 lanes x 2.4 GHz = 78.6e12 lane-ops/s
            vi = pmc["valu_insts_per_pair"]
            lane_ops = vi * 64.0 * pairs_per_launch / (fill_avg_ms * 1e-3)
            out["roofline_valu"] = {"bound": "valu", "achieved": lane_ops / 1e12, "peak": 78.6, "unit": "T lane-ops/s", "frac": lane_ops / 78.6e12,
                                    "valu_insts_per_pair": vi, "valu_busy": pmc.get("valu_busy"),
                                    "source": "SQ_INSTS_VALU, SQ_ACTIVE_INST_VALU, GRBM_GUI_ACTIVE (rocprofv3 --pmc, %s)" % os.path.basename(TRAFFIC_FILE)}
        if fast_path == 1 and args.series == "affine":
            # The BINDING ceiling of the headline sweep is VALU issue, not HBM: the floor of the recurrence is five
            # instructions per cell (add, max3, add, max, max), and tools/valu_ubench4.hip measured how fast a SIMD issues exactly that mix with
            # two or more waves resident: 1.813 ns per wave-instruction slot (profiles/r3_valu_ubench4.txt, "CELL int32 with add_sdwa").  A
            # read of n bases takes ceil(n / 8) rows in each of 8 lanes; 8 pairs share a wave; 4 SIMDs per CU.
            rr = 19 if READ_LEN <= 152 else 20
            slots_per_pair = CHUNK_LEN * rr * 5 / 8.0                      # wave-instruction slots of the floor
            n_simd = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
            floor_ms = pairs_per_launch * slots_per_pair * 1.813e-9 / n_simd * 1e3
            rv = out.setdefault("roofline_valu", {"bound": "valu"})
            rv.update({"floor_ms": floor_ms, "frac_of_floor": floor_ms / fill_avg_ms, "floor_model": "5 instructions per cell x 1.813 ns per wave-instruction slot and SIMD "
                       "(measured issue rate of add_sdwa, max3, add, max, max at >= 2 waves per SIMD, profiles/r3_valu_ubench4.txt) / (4 SIMDs x %d CUs)" % (n_simd // 4)})
        if args.full and not args.no_host and world == 1:
            # cold plans: a call of another shape first, so that the next full call builds and uploads its plans afresh
            step(max(n_pairs - 64, 1))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            out["cold_plan"] = {"ms_per_step": (time.perf_counter() - t1) * 1e3, "note": "one step after a call of another shape (no plan reuse)"}
            if host_timed:
                # the timed steps ARE host-entry calls; the library's own clock (entry to return) beside the driver-visible one
                same_h = same(fetch_device(n_pairs), got_main)
                ok = ok and same_h
                out["host_entry"] = {"entry": "gnx_align_batch_windows", "value": value, "unit": "DP cells/s", "ms_per_call": ms_per_step,
                                     "library_clock_ms": host_ms, "vs_device_resident": value / out["value_device_resident"],
                                     "equals_device_results": same_h,
                                     "includes": "H2D of reads, windows and offset tables, plans, kernels, D2H of scores / offsets / CIGAR runs into pinned host arrays (gnx_free)"}
                out["value_survey_8d"] = value  # (kept under its round-3 name: it is `value` now)
        if args.full and not args.no_extras and world == 1 and args.series == "affine":
            d_ops = None  # the extra legs need the memory (C3: 10 M reads of results on the device; C5: 70 GB of snapshots)
            torch.cuda.empty_cache()
            failed = []
            for name, fn in (("north_star_1M", extra_north_star), ("c3", extra_c3), ("c3_10M", extra_c3_10m), ("c5", extra_c5), ("n1", extra_n1), ("gsw_reads", extra_gsw), ("long_pairs", extra_long_pairs)):
                t1 = time.perf_counter()
                try:
                    out[name] = fn(_lib, L, scores, chunk_h, dev, torch)
                    ok = ok and out[name].get("bit_exact_sample", True)
                except Exception as e:  # an extra leg never takes the headline line down -- but it does clear bit_exact_sample
                    out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
                    failed.append(name)
                    ok = False
                out[name]["leg_wall_s"] = time.perf_counter() - t1
            out["extras_failed"] = failed
            _lib.check(L.gnx_init(dev_index, int(ws_gb * (1 << 30))))
        if args.full and not args.no_cpu and world == 1 and args.series in ("affine", "long"):
            cb = cpu_baseline(S, scores, pair_lists, n_pairs)
            exp, k = cb.pop("_oracle")
            # the oracle results of the baseline sample double as the bit-exactness check of the first k GPU results
            ok_k = same(fetch(k), exp)
            ok = ok and ok_k
            out["bit_exact_pairs_checked"] = int(max(k, min(n_verify, n_pairs)))
            out["cpu_baseline"] = cb
        out["bit_exact_sample"] = ok if checked else None
    # ---- N > 1: the one-process flow of the C ABI (gnx_init_devices) on the same GPUs, after every rank has given its memory back ----
    if world > 1 and S["shared"] and ((args.full and not args.no_extras and not args.share_gpu) or args.one_process):
        d_ops = d_score = d_off = d_reads = d_chunk = d_as = d_al = d_bs = d_bl = None  # (referenced by the closures above: release, do not del)
        L.gnx_shutdown()
        torch.cuda.empty_cache()
        dist.barrier()
        if rank == 0:
            t1 = time.perf_counter()
            try:
                out["one_process"] = one_process_flow(_lib, L, world, params, reads_h, chunk_h, n_pairs, same, args.steps, args.share_gpu)
                ok = ok and out["one_process"].get("bit_exact_sample", True)
            except Exception as e:
                out["one_process"] = {"error": "%s: %s" % (type(e).__name__, e)}
                ok = False
            out["one_process"]["leg_wall_s"] = time.perf_counter() - t1
            # a run on N distinct GPUs must have gone over RCCL with N ranks: a silent fall-back to peer copies does not pass as RCCL
            w = out["one_process"].get("windows", {})
            out["one_process"]["rccl_ok"] = bool(w.get("transport") == "rccl" and w.get("rccl_ranks") == world and out["one_process"].get("contexts") == world)
            out["one_process_rccl_ok"] = out["one_process"]["rccl_ok"]  # (reported, loudly; it does not change the exit code: the headline leg stands on its own)
            if not out["one_process"]["rccl_ok"] and not args.share_gpu:
                sys.stderr.write("bench.py: the one-process leg did NOT run over RCCL with %d ranks: %r\n" % (world, w.get("transport")))
            out["bit_exact_sample"] = ok
            L.gnx_shutdown()
        dist.barrier()
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()
    if not ok:
        sys.exit("bit-exactness check against the oracle FAILED")


if __name__ == "__main__":
    main()
