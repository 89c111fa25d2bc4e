// aln_summary.hip.h -- gnx_summarize_*: what is IN a finished alignment (contract: gnx_align.h)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).
//
// A CIGAR is walked against its two sequences: identities and substitutions among the M columns, gap bases and gap runs, the column
// re-score (scoreAffineAln's rule), the =/X form of the CIGAR.  No DP: every field is a sum over columns or a value carried along them.
//
// Geometry of aln_summary_kernel: one wave per pair, four pairs per workgroup (revcomp_reads_kernel's), no LDS, no scratch, no atomics.  The wave takes the
// CIGAR in blocks of 64 runs: every lane loads one run (16 bytes: one coalesced 1 KB read), three wave scans (__shfl_up) of the runs'
// rows / columns / lengths give each run its origin (i, j) and its first column index, and the totals carry to the next block as
// wave-uniform values.  A sequence holds fewer than 2^30 bases (the host checks it, as the align entries do), so positions are int,
// column indices and run counts unsigned; only the score sum is 64 bits wide.
//
// The seam rule.  n_xops and gap_runs both count RUN STARTS: columns whose extended type (I, D, =, X) differs from the type of the
// column before.  The type of the column before a run's first column is a function of POSITION alone: the op of the nearest run of
// non-zero length before it (found with one ballot; across blocks: a carried op), and, when that run is an M run, the equality of the
// two bases at (i - 1, j - 1), which the lane loads itself.  So a run's starts do not depend on who walked the runs before it, zero-length
// runs and equal adjacent ops fall out (a zero-length run has no column and is nobody's predecessor; a D run behind a D run starts
// nothing), and run starts are additive over runs, 64-column steps and 64-run blocks.
//
// Two forms of walking a block's M runs; every result is an integer sum, so it cannot depend on which form ran:
//   lane per run      each lane walks its own M run column by column (I and D runs need no walk: one start or none).
//   lane per column   an M run of at least `cut` columns is walked by the whole wave: origin and length made wave-uniform
//                     (__shfl from the owning lane), 64 columns per step, equality as one ballot and a population count, run starts
//                     as (eq ^ (eq << 1 | carried bit)), the matrix score of each lane's column accumulated per lane.
// The cut is 64 columns: a run shorter than one step leaves lanes idle in the lane-per-column form, while 64 lanes walking 64 short
// runs of their own keep all of them busy.  GNX_SUMMARY_FORM=0 sends every M run to the lane-per-column form, =1 every one to the
// lane-per-run form (tests).  Per-lane sums (equal columns, gap starts, scores) are reduced once per pair; the M / I / D base counts
// follow from the carried totals.
//
// The free end gaps of AffineGapLocal (the leading and the trailing maximal D run) are read off the two ends of the CIGAR after the
// walk (sum_free_end: one block of runs each unless an end holds more than 64 D / empty runs) and un-charged from the totals once.
//
// Extended CIGAR: the summary pass (WRITE = false) yields n_xops per pair, scan_kernel's family turns them into offsets, and the
// WRITE instantiation walks again: per block it counts the starts of every run, scans the counts into output slots and walks once
// more; each run start closes the run BEFORE it (slot k - 1 = {start column - previous start column, type before}), the last run is
// closed after the last block.  The previous start column comes from a max scan over the lanes, like the slot from the sum scan
// (start columns are carried plus one, 0 = no start yet).
//
// Either sequence may be plain bytes or a window of the packed resident reference (BetaSrcT, 16 bases per dword, exception path
// for blocks with N): _by_offset reads the reference where the mode puts it (beta in the global modes, alpha = the target in
// AffineGapLocal) and never unpacks a window.
#pragma once
#include "gnx_common.hip.h"

namespace {

struct SumArgs {
    KParams kp;     // only the packed-reference pointers are read, by the side the kernel's PK names (1: alpha, 2: beta, 0: neither: plain bytes in a_buf / b_buf)
    const uint8_t *a_buf, *b_buf;
    const int64_t *a_start, *a_len, *b_start, *b_len;
    const gnx_cigar *ops;
    const int64_t *ops_off; // absolute, ops_off[p] .. ops_off[p + 1]
    const int64_t *scores;  // 25 entries, device memory
    int64_t gap_open, gap_extend;
    int64_t n_pairs;
    int cut;                // M runs of at least this many columns take the lane-per-column form
    int affine, local;
    int slice;              // aln_summary_bases_kernel: bases of either sequence per workgroup of a pair (a multiple of 256)
    gnx_aln_summary *out;   // WRITE = false
    int64_t *nx;            // WRITE = false: n_xops per pair, contiguous for the scan
    int *err;               // bit 0: a base >= 5
    const int64_t *xoff;    // WRITE = true: first slot of each pair
    gnx_cigar *xops;
};

__device__ __forceinline__ int64_t sum_wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned sum_wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// exclusive sum scan over the lanes; total = the wave's sum
__device__ __forceinline__ unsigned sum_wave_scan(unsigned v, int lane, unsigned &total) {
    unsigned s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(s, d, 64); if (lane >= d) s += t; }
    total = __shfl(s, 63, 64);
    return s - v;
}
// exclusive max scan over the lanes on top of `carry`; total = max(carry, every lane)
__device__ __forceinline__ unsigned sum_wave_maxscan(unsigned v, int lane, unsigned carry, unsigned &total) {
    unsigned s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(s, d, 64); if (lane >= d) s = max(s, t); }
    total = max(carry, (unsigned)__shfl(s, 63, 64));
    const unsigned e = __shfl_up(s, 1, 64);
    return lane == 0 ? carry : max(carry, e);
}
__device__ __forceinline__ int64_t sum_score(const int64_t *sc, int x, int y) { return sc[min(x, 4) * 5 + min(y, 4)]; } // (a byte >= 5 fails the call: no read past the table)
__device__ __forceinline__ void sum_emit(gnx_cigar *xo, unsigned slot, unsigned len, int type) {
    gnx_cigar r;
    r.run_length = (int64_t)len; r.op = (uint8_t)type;
#pragma unroll
    for (int q = 0; q < 7; q++) r._pad[q] = 0;
    xo[slot] = r;
}

// what a walk of one run yields: its run starts, the column of the last one plus one (0: none), its equal columns, the sum of its matrix scores
struct SumRun { unsigned cnt, last1, eq; int64_t sc; };

// lane per run: this lane's M run of `len` columns from (i0, j0), first column index c0, the type before it `pred`
// EMIT: slot = the index of this run's first start, ps1 = the start column before it, plus one
template <bool EMIT, bool SUMS, class SrcA, class SrcB>
__device__ __forceinline__ SumRun sum_walk_run(const SrcA &A, const SrcB &B, const int64_t *sc, int i0, int j0, unsigned c0, int len, int pred,
                                               gnx_cigar *xo, unsigned slot, unsigned ps1) {
    SumRun r = {0, 0, 0, 0};
    int t = pred;
    // the bases of a column are loaded one column ahead, its matrix entry is added one column later: the lane's loads overlap
    int x = A.at(i0), y = B.at(j0);
    int64_t pend = 0;
    for (int k = 0; k < len; k++) {
        int nx = 0, ny = 0;
        if (k + 1 < len) { nx = A.at(i0 + k + 1); ny = B.at(j0 + k + 1); }
        const int ty = x == y ? GNX_XCOL_EQ : GNX_XCOL_X;
        if (ty != t) {
            if (EMIT) { if (t >= 0) sum_emit(xo, slot + r.cnt - 1, c0 + k + 1 - ps1, t); ps1 = c0 + k + 1; }
            r.cnt++; r.last1 = c0 + k + 1;
        }
        t = ty;
        if (SUMS) { r.eq += x == y; r.sc += pend; pend = sum_score(sc, x, y); }
        x = nx; y = ny;
    }
    if (SUMS) r.sc += pend;
    return r;
}

// lane per column: the same run, every argument wave-uniform; eq and sc come back PER LANE (the caller's accumulators), cnt / last1 uniform
template <bool EMIT, bool SUMS, class SrcA, class SrcB>
__device__ __forceinline__ SumRun sum_walk_wave(const SrcA &A, const SrcB &B, const int64_t *sc, int i0, int j0, unsigned c0, int len, int pred, int lane,
                                                gnx_cigar *xo, unsigned slot, unsigned ps1) {
    SumRun r = {0, 0, 0, 0};
    int t = pred; // type of the column before this step's lane 0
    const unsigned long long below = (1ull << lane) - 1ull;
    // the bases of a step are loaded one step ahead: one wave walks the whole run, and nothing else hides the latency of its loads
    bool valid = lane < len;
    int x = 0, y = 0;
    if (valid) { x = A.at(i0 + lane); y = B.at(j0 + lane); }
    int64_t pend = 0;
    for (int s = 0; s < len; s += 64) {
        const int k = s + lane;
        const bool nvalid = k + 64 < len;
        int nx = 0, ny = 0;
        if (nvalid) { nx = A.at(i0 + k + 64); ny = B.at(j0 + k + 64); }
        const unsigned long long vm = __ballot(valid), em = __ballot(valid && x == y);
        const unsigned long long sm = ((em ^ ((em << 1) | (t == GNX_XCOL_EQ ? 1ull : 0ull))) | ((t == GNX_XCOL_EQ || t == GNX_XCOL_X) ? 0ull : 1ull)) & vm;
        const unsigned top1 = sm ? c0 + s + (64 - __clzll((long long)sm)) : 0; // the step's last start column, plus one
        if (EMIT) {
            if ((sm >> lane) & 1ull) {
                const unsigned long long pm = sm & below;
                const int tb = lane == 0 ? t : (((em >> (lane - 1)) & 1ull) ? GNX_XCOL_EQ : GNX_XCOL_X);
                const unsigned before1 = pm ? c0 + s + (64 - __clzll((long long)pm)) : ps1;
                if (tb >= 0) sum_emit(xo, slot + r.cnt + __popcll(pm) - 1, c0 + k + 1 - before1, tb);
            }
            if (sm) ps1 = top1;
        }
        if (SUMS) { r.sc += pend; pend = 0; if (valid) { r.eq += x == y; pend = sum_score(sc, x, y); } } // (the matrix entry is added a step later)
        if (sm) r.last1 = top1;
        r.cnt += __popcll(sm);
        t = ((em >> (63 - __clzll((long long)vm))) & 1ull) ? GNX_XCOL_EQ : GNX_XCOL_X;
        x = nx; y = ny; valid = nvalid;
    }
    if (SUMS) r.sc += pend;
    return r;
}

// AffineGapLocal's free end gap at one end of a CIGAR: the D bases of the maximal D run there (zero-length runs skipped).  Lane 0 takes
// the outermost run; the walk ends with the first block that holds a column that is not D -- as a rule the first.
__device__ __forceinline__ unsigned sum_free_end(const gnx_cigar *ops, int64_t nr, int lane, bool tail) {
    unsigned total = 0;
    for (int64_t rb = 0; rb < nr; rb += 64) {
        const int64_t x = tail ? nr - 1 - rb - lane : rb + lane;
        int len = 0, op = 0;
        if (x >= 0 && x < nr) { const gnx_cigar run = ops[x]; len = (int)run.run_length; op = run.op; }
        const unsigned long long nd = __ballot(len > 0 && op != GNX_COL_D);
        const unsigned long long fm = nd ? ((1ull << (__ffsll((long long)nd) - 1)) - 1ull) : ~0ull;
        total += sum_wave_sum(((fm >> lane) & 1ull) && op == GNX_COL_D ? (unsigned)len : 0u);
        if (nd) break;
    }
    return total;
}

// GNX_EBASE where the align twin reports it: a byte >= 5 anywhere in either sequence of a pair, consumed by the CIGAR or not (a packed
// window without exception blocks holds none and is not read).  A kernel of its own: the walk below reads only the M columns, and with
// these loops unrolled inside it the walk ran out of scalar registers.  The gridDim.y workgroups of a pair take `slice` consecutive
// bases of either sequence each (the host asks for more than one when the launch is a few long pairs: a megabase pair is not one
// workgroup's work).
template <int PK>
__global__ __launch_bounds__(256) void aln_summary_bases_kernel(SumArgs a) {
    const int lo = (int)blockIdx.y * a.slice;
    for (int64_t p = blockIdx.x; p < a.n_pairs; p += gridDim.x) {
        const int n = (int)a.a_len[p], m = (int)a.b_len[p];
        BetaSrcT<PK == 1 ? 1 : 0> A;
        BetaSrcT<PK == 2 ? 1 : 0> B;
        A.init(a.a_buf, a.kp, a.a_start[p], n);
        B.init(a.b_buf, a.kp, a.b_start[p], m);
        bool bad = false;
        if (!A.packed() || A.dirty) for (int k = lo + (int)threadIdx.x; k < min(n, lo + a.slice); k += 256) bad |= A.at(k) >= 5;
        if (!B.packed() || B.dirty) for (int k = lo + (int)threadIdx.x; k < min(m, lo + a.slice); k += 256) bad |= B.at(k) >= 5;
        if (bad) *a.err = 1; // (every writer stores the same value: no atomic)
    }
}

// PK: which side is a window of the packed reference (known at compile time: the byte side then carries no packed-reference state)
template <bool WRITE, int PK>
__global__ __launch_bounds__(256) void aln_summary_kernel(SumArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += (int64_t)gridDim.x * 4) {
        const int n = (int)a.a_len[p], m = (int)a.b_len[p];
        BetaSrcT<PK == 1 ? 1 : 0> A;
        BetaSrcT<PK == 2 ? 1 : 0> B;
        A.init(a.a_buf, a.kp, a.a_start[p], n);
        B.init(a.b_buf, a.kp, a.b_start[p], m);
        const int64_t r0 = a.ops_off[p], nr = a.ops_off[p + 1] - r0;
        gnx_cigar *xo = WRITE ? a.xops + a.xoff[p] : nullptr;
        // carried from block to block, wave-uniform
        unsigned ci = 0, cj = 0, cc = 0;    // alpha bases, beta bases, columns so far
        int prev_op = -1;                   // op of the last run of non-zero length (-1: none yet)
        unsigned n_starts = 0, last1 = 0;   // run starts so far, the column of the last one plus one
        // per lane, reduced once per pair
        unsigned acc_eq = 0, acc_gap = 0;
        int64_t acc_sc = 0;
        int nlen = 0, nop = 0; // the next block's runs, loaded one block ahead
        if (lane < nr) { const gnx_cigar run = a.ops[r0 + lane]; nlen = (int)run.run_length; nop = run.op; }
        for (int64_t rb = 0; rb < nr; rb += 64) {
            const int len = nlen, op = nop;
            nlen = 0; nop = 0;
            if (rb + 64 + lane < nr) { const gnx_cigar run = a.ops[r0 + rb + 64 + lane]; nlen = (int)run.run_length; nop = run.op; }
            unsigned ti, tj, tc;
            const int i0 = (int)(ci + sum_wave_scan(op != GNX_COL_I ? (unsigned)len : 0u, lane, ti));
            const int j0 = (int)(cj + sum_wave_scan(op != GNX_COL_D ? (unsigned)len : 0u, lane, tj));
            const unsigned c0 = cc + sum_wave_scan((unsigned)len, lane, tc);
            const unsigned long long nz = __ballot(len > 0);
            // the type of the column before this run's first column (the seam rule)
            const unsigned long long nzb = nz & below;
            int pop = __shfl(op, nzb ? 63 - __clzll((long long)nzb) : 0, 64);
            if (!nzb) pop = prev_op;
            int pred = pop;
            if (len > 0 && pop == GNX_COL_M) pred = A.at(i0 - 1) == B.at(j0 - 1) ? GNX_XCOL_EQ : GNX_XCOL_X;
            const bool gap = len > 0 && op != GNX_COL_M, mrun = len > 0 && op == GNX_COL_M, coop = mrun && len >= a.cut;
            // pass 1: the starts of every run
            SumRun r = {0, 0, 0, 0};
            if (gap && pred != op) { r.cnt = 1; r.last1 = c0 + 1; }
            if (mrun && !coop) r = sum_walk_run<false, !WRITE>(A, B, a.scores, i0, j0, c0, len, pred, nullptr, 0, 0);
            const unsigned long long cm0 = __ballot(coop);
            for (unsigned long long cm = cm0; cm; cm &= cm - 1) {
                const int o = __ffsll((long long)cm) - 1;
                const SumRun u = sum_walk_wave<false, !WRITE>(A, B, a.scores, __shfl(i0, o, 64), __shfl(j0, o, 64), __shfl(c0, o, 64), __shfl(len, o, 64), __shfl(pred, o, 64), lane,
                                                              nullptr, 0, 0);
                if (!WRITE) { acc_eq += u.eq; acc_sc += u.sc; }
                if (lane == o) { r.cnt = u.cnt; r.last1 = u.last1; }
            }
            if (!WRITE) {
                acc_eq += r.eq; acc_sc += r.sc;
                if (gap && pred != op) acc_gap++;
            }
            unsigned tcnt;
            const unsigned slot = n_starts + sum_wave_scan(r.cnt, lane, tcnt);
            if (WRITE) { // pass 2: every start closes the run before it
                unsigned tlast;
                const unsigned ps1 = sum_wave_maxscan(r.last1, lane, last1, tlast);
                if (gap && pred != op && pred >= 0) sum_emit(xo, slot - 1, c0 + 1 - ps1, pred);
                if (mrun && !coop) (void)sum_walk_run<true, false>(A, B, a.scores, i0, j0, c0, len, pred, xo, slot, ps1);
                for (unsigned long long cm = cm0; cm; cm &= cm - 1) {
                    const int o = __ffsll((long long)cm) - 1;
                    (void)sum_walk_wave<true, false>(A, B, a.scores, __shfl(i0, o, 64), __shfl(j0, o, 64), __shfl(c0, o, 64), __shfl(len, o, 64), __shfl(pred, o, 64), lane, xo,
                                                     __shfl(slot, o, 64), __shfl(ps1, o, 64));
                }
                last1 = tlast;
            }
            n_starts += tcnt;
            ci += ti; cj += tj; cc += tc;
            if (nz) prev_op = __shfl(op, 63 - __clzll((long long)nz), 64);
        }
        if (WRITE) {
            if (lane == 0 && n_starts > 0) {
                int t = prev_op;
                if (t == GNX_COL_M) t = A.at((int)ci - 1) == B.at((int)cj - 1) ? GNX_XCOL_EQ : GNX_XCOL_X;
                sum_emit(xo, n_starts - 1, cc + 1 - last1, t);
            }
            continue;
        }
        // ci = M + D, cj = M + I, cc = M + I + D columns
        const int64_t n_eq = sum_wave_sum(acc_eq), n_m = (int64_t)ci + cj - cc, ins = (int64_t)cc - ci, sc = sum_wave_sum(acc_sc);
        int64_t del = (int64_t)cc - cj, gaps = sum_wave_sum(acc_gap), a_start = 0, a_end = ci;
        if (a.local) {
            const unsigned lead = sum_free_end(a.ops + r0, nr, lane, false), trail = sum_free_end(a.ops + r0, nr, lane, true);
            if (cc > 0 && lead == cc) { del = 0; gaps = 0; a_end = 0; } // one D run: free as a whole, start = end = 0
            else { del -= (int64_t)lead + trail; gaps -= (lead > 0) + (trail > 0); a_start = lead; a_end = (int64_t)ci - trail; }
        }
        if (lane == 0) {
            gnx_aln_summary s;
            s.rescore = sc + (a.affine ? a.gap_open * gaps + a.gap_extend * (ins + del) : a.gap_open * (ins + del));
            s.alpha_used = ci; s.beta_used = cj; s.alpha_start = a_start; s.alpha_end = a_end;
            s.n_equal = n_eq; s.n_mismatch = n_m - n_eq; s.ins_bases = ins; s.del_bases = del; s.gap_runs = gaps; s.n_xops = n_starts; s._reserved = 0;
            a.out[p] = s;
            a.nx[p] = n_starts;
        }
    }
}

} // namespace
