// pileup.hip.h -- gnx_pileup_*: what the placed reads, taken together, say about each reference position (contract: gnx_align.h)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).
//
// The pile is a table beside the resident reference: for every position of a region, how many read bases of each letter lie over it in
// M columns, how many D columns, and how many I runs stand directly behind it, per strand.  pile_add_kernel adds finished alignments to
// it, pile_call_kernel turns it into a sparse list of the positions where the reads disagree with the reference.
//
// Layout: PILE_PLANES planes of region_len int32 counters (plane = strand * 5 + base, PILE_DEL + strand, PILE_INS + strand), not rows
// of 16 counters.  In the lane-per-column form a wave's 64 adds fall on 64 consecutive counters of at most five planes -- 256 contiguous
// bytes per plane touched --, where rows would send every lane to a 64-byte row of its own.  gnx_pileup_get transposes on the host.
//
// Geometry of pile_add_kernel: aln_summary_kernel's -- one wave per pair, four pairs per workgroup, the CIGAR in blocks of 64 runs loaded
// a block ahead, wave scans (sum_wave_scan) of the runs' alpha and beta bases giving every run its origin (i, j), totals carried from
// block to block as wave-uniform values; no LDS, no scratch.  No reference read: the position, the read byte and the strand decide every
// add.  A column index is not needed either: whether a run is inside (AffineGapLocal's leading and trailing maximal D run are not) is a
// function of its alpha origin -- the pieces of the leading D run start before alpha_start, those of the trailing one at or behind
// alpha_end, every other run in between -- so alpha_start (sum_free_end) and alpha_end (the alpha total minus sum_free_end at the tail)
// are taken BEFORE the walk, as aln_md_kernel takes them, in one pass over the run lengths.
// An I run is counted once, where it starts: at a run of non-zero length whose predecessor -- the summary's seam rule: the op of the
// nearest run of non-zero length before it, carried across blocks -- is not an I run.  It stands behind i consumed alpha bases and
// counts at i - 1 when alpha_start < i < alpha_end (an I run at either end is a soft clip and counts nowhere).
//
// Two forms of walking a run, as in the summary; the counters are integer sums, so they cannot depend on which ran:
//   lane per run      each lane walks its own M or D run column by column.
//   lane per column   a run of at least `cut` columns is taken by the whole wave, 64 columns per step.
// The cut is 64 columns.  GNX_PILE_FORM=0 sends every run to the lane-per-column form, =1 every one to the lane-per-run form (tests).
// Counters are bumped with atomicAdd whose result is not used (global_atomic_add_u32 without return).  A call adds at most 1 per read to
// a counter and the host keeps the reads added below 2^31: no counter overflows.
//
// pile_call_kernel<WRITE>: one position per lane, PILE_TILE positions per wave in steps of 64; the 14 counters (one coalesced read per
// plane) and the reference code through BetaSrcT<1> (16 bases per dword, the exception path for blocks with N).  The count / scan /
// write pattern of the extended CIGAR and of MD: WRITE = false leaves the calls of each tile, scan_kernel's family turns them into
// offsets, WRITE = true decides again and stores, a wave scan giving each lane its slot behind the tile's offset.
#pragma once
#include "aln_summary.hip.h"

namespace {

constexpr int PILE_PLANES = 14; // base[2][5], del[2], ins[2]
constexpr int PILE_DEL = 10, PILE_INS = 12;
constexpr int PILE_TILE = 256;  // positions per wave of pile_call_kernel: one entry of the scanned array

struct PileArgs {
    const uint8_t *reads;      // the reads one behind the other, each in the orientation it was aligned in
    const int64_t *read_start; // per pair: its first byte in `reads`
    const int64_t *ref_start;  // per pair: the reference position of its window's first base
    const gnx_cigar *ops;
    const int64_t *ops_off;    // absolute, ops_off[p] .. ops_off[p + 1]
    const uint8_t *strand;     // per pair: 0 / 1, picks the counter
    const uint8_t *use;        // per pair: 0 = leave it out; nullptr: all
    int64_t n_pairs;
    int cut;                   // runs of at least this many columns take the lane-per-column form
    int *pile;                 // PILE_PLANES planes of region_len counters
    int64_t region_start, region_len;
};

// one pair's view of the table: alpha position i lies over region position x0 + i, inside the region for lo <= i < hi
struct PileWin { int *pile; int64_t len, x0; int lo, hi; };
__device__ __forceinline__ void pile_bump(const PileWin &w, int plane, int i) {
    if (i >= w.lo && i < w.hi) (void)atomicAdd(w.pile + ((int64_t)plane * w.len + (w.x0 + i)), 1);
}

__global__ __launch_bounds__(256) void pile_add_kernel(PileArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += (int64_t)gridDim.x * 4) {
        if (a.use && !a.use[p]) continue;
        const int64_t r0 = a.ops_off[p], nr = a.ops_off[p + 1] - r0;
        const uint8_t *rd = a.reads + a.read_start[p];
        const int sg = a.strand[p] ? 1 : 0, sb = 5 * sg;
        PileWin w;
        w.pile = a.pile; w.len = a.region_len; w.x0 = a.ref_start[p] - a.region_start;
        const int64_t top = (int64_t)1 << 30; // (a sequence holds fewer bases: the host checks it)
        const int64_t lo = -w.x0, hi = a.region_len - w.x0;
        w.lo = lo < 0 ? 0 : lo > top ? (int)top : (int)lo; w.hi = hi < 0 ? 0 : hi > top ? (int)top : (int)hi;
        // the inside alpha positions: [a_start, a_end) (one D run: a_start = the alpha total, a_end = 0, nothing inside)
        unsigned alpha = 0;
        for (int64_t rb = 0; rb < nr; rb += 64) {
            unsigned v = 0;
            if (rb + lane < nr) { const gnx_cigar run = a.ops[r0 + rb + lane]; v = run.op != GNX_COL_I ? (unsigned)run.run_length : 0u; }
            alpha += sum_wave_sum(v);
        }
        const unsigned a_start = sum_free_end(a.ops + r0, nr, lane, false), a_end = alpha - sum_free_end(a.ops + r0, nr, lane, true);
        // carried from block to block, wave-uniform
        unsigned ci = 0, cj = 0; // alpha bases, beta bases so far
        int prev_op = -1;        // op of the last run of non-zero length (-1: none yet)
        int nlen = 0, nop = 0;   // the next block's runs, loaded one block ahead
        if (lane < nr) { const gnx_cigar run = a.ops[r0 + lane]; nlen = (int)run.run_length; nop = run.op; }
        for (int64_t rb = 0; rb < nr; rb += 64) {
            const int len = nlen, op = nop;
            nlen = 0; nop = 0;
            if (rb + 64 + lane < nr) { const gnx_cigar run = a.ops[r0 + rb + 64 + lane]; nlen = (int)run.run_length; nop = run.op; }
            unsigned ti, tj;
            const int i0 = (int)(ci + sum_wave_scan(op != GNX_COL_I ? (unsigned)len : 0u, lane, ti));
            const int j0 = (int)(cj + sum_wave_scan(op != GNX_COL_D ? (unsigned)len : 0u, lane, tj));
            const unsigned long long nz = __ballot(len > 0);
            // the op of the column before this run's first column (the seam rule)
            const unsigned long long nzb = nz & below;
            int pop = __shfl(op, nzb ? 63 - __clzll((long long)nzb) : 0, 64);
            if (!nzb) pop = prev_op;
            const bool mrun = len > 0 && op == GNX_COL_M;
            const bool drun = len > 0 && op == GNX_COL_D && (unsigned)i0 >= a_start && (unsigned)i0 < a_end;
            if (len > 0 && op == GNX_COL_I && pop != GNX_COL_I && (unsigned)i0 > a_start && (unsigned)i0 < a_end) pile_bump(w, PILE_INS + sg, i0 - 1);
            const bool coop = (mrun || drun) && len >= a.cut;
            if ((mrun || drun) && !coop) { // lane per run
                if (mrun) for (int k = 0; k < len; k++) pile_bump(w, sb + min((int)rd[j0 + k], 4), i0 + k); // (a byte >= 5 fails the call before this kernel runs)
                else for (int k = 0; k < len; k++) pile_bump(w, PILE_DEL + sg, i0 + k);
            }
            for (unsigned long long cm = __ballot(coop); cm; cm &= cm - 1) { // lane per column
                const int o = __ffsll((long long)cm) - 1;
                const int ui0 = __shfl(i0, o, 64), uj0 = __shfl(j0, o, 64), ulen = __shfl(len, o, 64);
                if (__shfl(op, o, 64) == GNX_COL_M) for (int k = lane; k < ulen; k += 64) pile_bump(w, sb + min((int)rd[uj0 + k], 4), ui0 + k);
                else for (int k = lane; k < ulen; k += 64) pile_bump(w, PILE_DEL + sg, ui0 + k);
            }
            ci += ti; cj += tj;
            if (nz) prev_op = __shfl(op, 63 - __clzll((long long)nz), 64);
        }
    }
}

struct PileCallArgs {
    KParams kp;        // only the packed-reference pointers are read
    const int *pile;
    int64_t region_start, region_len, n_tiles;
    int min_depth, min_alt, frac_num, frac_den, both_strands;
    int64_t *cnt;       // WRITE = false: the calls of each tile, contiguous for the scan
    const int64_t *off; // WRITE = true: first slot of each tile
    gnx_pile_call *out;
};

__device__ __forceinline__ bool pile_passes(const PileCallArgs &a, int depth, int count, int fwd) {
    return depth >= a.min_depth && count >= a.min_alt && (int64_t)count * a.frac_den >= (int64_t)a.frac_num * depth && (!a.both_strands || (fwd >= 1 && count - fwd >= 1));
}
__device__ __forceinline__ void pile_emit(gnx_pile_call *out, int64_t slot, int64_t pos, int depth, int count, int fwd, int kind, int ref, int alt) {
    gnx_pile_call c;
    c.pos = pos; c.depth = depth; c.count = count; c.count_fwd = fwd;
    c.kind = (uint8_t)kind; c.ref = (uint8_t)ref; c.alt = (uint8_t)alt; c._pad = 0;
    out[slot] = c;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void pile_call_kernel(PileCallArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < a.n_tiles; t += (int64_t)gridDim.x * 4) {
        int64_t n_tile = WRITE ? a.off[t] : 0; // calls of the tile so far (WRITE: on top of its first slot)
        for (int s = 0; s < PILE_TILE; s += 64) {
            const int64_t r = t * PILE_TILE + s; // the step's first position in the region
            if (r >= a.region_len) break;
            const int nv = a.region_len - r < 64 ? (int)(a.region_len - r) : 64;
            BetaSrcT<1> R;
            R.init(nullptr, a.kp, a.region_start + r, nv);
            int depth = 0, pc = -1, pf = 0, pa = 0, ic = 0, ifw = 0, c = 4;
            bool prim = false, insc = false;
            if (lane < nv) {
                c = R.at(lane);
                const int *q = a.pile + (r + lane);
                const int64_t L = a.region_len;
                const int del_f = q[PILE_DEL * L], del_r = q[(PILE_DEL + 1) * L];
                depth = q[4 * L] + q[9 * L] + del_f + del_r;
#pragma unroll
                for (int b = 0; b < 4; b++) { // the candidates in order: ties go to the smaller index, the deletion last
                    const int f = q[b * L], n = f + q[(5 + b) * L];
                    depth += n;
                    if (b != c && n > pc) { pc = n; pf = f; pa = b; }
                }
                if (del_f + del_r > pc) { pc = del_f + del_r; pf = del_f; pa = 4; }
                ifw = q[PILE_INS * L]; ic = ifw + q[(PILE_INS + 1) * L];
                prim = c < 4 && pile_passes(a, depth, pc, pf);
                insc = c < 4 && pile_passes(a, depth, ic, ifw);
            }
            const unsigned mine = (prim ? 1u : 0u) + (insc ? 1u : 0u);
            if (WRITE) {
                unsigned total;
                const int64_t slot = n_tile + sum_wave_scan(mine, lane, total);
                const int64_t pos = a.region_start + r + lane;
                if (prim) pile_emit(a.out, slot, pos, depth, pc, pf, pa == 4 ? 1 : 0, c, pa == 4 ? 0xFF : pa);
                if (insc) pile_emit(a.out, slot + (prim ? 1 : 0), pos, depth, ic, ifw, 2, c, 0xFF);
                n_tile += total;
            } else n_tile += sum_wave_sum(mine);
        }
        if (!WRITE && lane == 0) a.cnt[t] = n_tile;
    }
}

} // namespace
