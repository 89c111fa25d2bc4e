// pile_alleles.hip.h -- the alleles of the pile: WHICH deletion, WHICH insertion (contract: gnx_align.h)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit) beside pileup.hip.h.
//
// A tracking pile (gnx_pileup_track_alleles) keeps, beside its planes, a log of indel events: one per maximal inside D run (its first
// deleted base, its length) and one per maximal inside I run that bumps `ins` (the base it stands behind, its bases).  The reads and CIGARs
// are on the device only during gnx_pileup_add_by_offset, so allele_log_kernel runs there, a second launch per sub-batch over the buffers
// pile_add_kernel has just read.  pile_add_kernel itself is untouched; a pile that does not track launches exactly what it launched before.
//
// An event is 16 bytes, two 8-byte words kept in two planes of the log (w0 of every event, then w1 of every event) as the pile's counters
// are planes: rocprim::radix_sort_pairs takes keys and values as separate arrays, so the query sorts the log as it lies.
//   w0 = (pos - region_start) << 2 | kind      kind 1 deletion, 2 insertion of <= 21 bases, 3 longer insertion
//   w1 = key << 1 | strand                     key = the length (kinds 1, 3) or the packed bases (kind 2: 3 bits a base, code + 1, the first
//                                              base lowest, a read N = 5; 21 bases are the 63 bits that the strand bit leaves)
//
// Geometry of allele_log_kernel: pile_add_kernel's -- one wave per pair, four per workgroup, runs in blocks of 64 loaded a block ahead,
// sum_wave_scan for the alpha / beta origin of every run, alpha_start / alpha_end before the walk.  It touches runs, not columns: one lane
// per run.  An event belongs to a MAXIMAL run, which may come as several pieces (adjacent equal ops, zero-length runs of other ops in
// between, across one or more block seams).  With the seam rule of pile_add_kernel a lane knows the op before its run; a run of non-zero
// length whose predecessor has another op is a segment HEAD.  A head opens its own segment and CLOSES the one before it, and what it needs
// of that one is a difference of scan values: a D segment's length is the alpha consumed between the two heads, an I segment's the beta
// consumed -- the exclusive scans ARE the segmented sum over the heads' ballot.  The head before is the highest head bit below the lane
// (one shuffle), or, when the block holds none below, the open segment carried wave-uniform from block to block (op, alpha origin, beta
// origin: the length so far is implied).  A segment still open at the end of the CIGAR is a trailing D run or a terminal I run and is
// never recorded; the leading D run is closed but starts before alpha_start.  The lane that closes an insertion packs its read bytes.
// Events are appended wave-aggregated: ballot, ONE returned atomicAdd on the log's cursor per wave and block by one lane, slot by the
// population count below.  No hash table, no wave waits for another, no LDS, no scratch.  The host sized the log for every non-zero I and D
// run of the call before the first launch; `cap` is checked all the same and nothing is stored behind it.
//
// Query (gnx_pileup_alleles): two stable radix sorts of the log's copy, by w1 and then by w0, give the order (pos, kind, key, strand).
// allele_reduce_kernel<WRITE> is the project's count / scan / write pattern: an entry is a group head where (w0, w1 >> 1) differs
// from the entry before; WRITE = false counts the heads of each tile of PILE_TILE entries, the scan family turns them into offsets, WRITE =
// true stores one gnx_pile_allele per head.  The sorted array is ordered by (w0, w1) as a whole, so a head finds the end of its group and
// the end of its strand-0 part with two binary searches, whatever the group's size.  The log itself stays raw: the query changes nothing.
// allele_call_kernel<WRITE>: one allele per lane from the device array the reduce left, the 12 depth counters of its position from the
// planes, the reference code through BetaSrcT<1>, pile_call_kernel's four tests; count / scan / write keeps the alleles' order.
#pragma once
#include "pileup.hip.h"

namespace {

constexpr int PILE_SEQ_MAX = 21; // inserted bases whose sequence is kept: 63 bits at 3 bits a base

struct PileAlleleArgs {
    const uint8_t *reads;
    const int64_t *read_start, *ref_start;
    const gnx_cigar *ops;
    const int64_t *ops_off;
    const uint8_t *strand, *use;
    int64_t n_pairs;
    int64_t region_start, region_len;
    unsigned long long *w0, *w1; // the log's planes
    unsigned long long *cursor;  // events in the log
    unsigned long long cap;      // events the planes hold
};

__global__ __launch_bounds__(256) void allele_log_kernel(PileAlleleArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += (int64_t)gridDim.x * 4) {
        if (a.use && !a.use[p]) continue;
        const int64_t r0 = a.ops_off[p], nr = a.ops_off[p + 1] - r0;
        const uint8_t *rd = a.reads + a.read_start[p];
        const unsigned long long sg = a.strand[p] ? 1ull : 0ull;
        const int64_t x0 = a.ref_start[p] - a.region_start; // alpha position i lies over region position x0 + i
        unsigned alpha = 0;
        for (int64_t rb = 0; rb < nr; rb += 64) {
            unsigned v = 0;
            if (rb + lane < nr) { const gnx_cigar run = a.ops[r0 + rb + lane]; v = run.op != GNX_COL_I ? (unsigned)run.run_length : 0u; }
            alpha += sum_wave_sum(v);
        }
        const unsigned a_start = sum_free_end(a.ops + r0, nr, lane, false), a_end = alpha - sum_free_end(a.ops + r0, nr, lane, true);
        // carried from block to block, wave-uniform
        unsigned ci = 0, cj = 0;     // alpha bases, beta bases so far
        int seg_op = -1;             // the open segment: the op of the last run of non-zero length (-1: none yet) ...
        unsigned seg_i = 0, seg_j = 0; // ... and the origin of its head
        int nlen = 0, nop = 0;
        if (lane < nr) { const gnx_cigar run = a.ops[r0 + lane]; nlen = (int)run.run_length; nop = run.op; }
        for (int64_t rb = 0; rb < nr; rb += 64) {
            const int len = nlen, op = nop;
            nlen = 0; nop = 0;
            if (rb + 64 + lane < nr) { const gnx_cigar run = a.ops[r0 + rb + 64 + lane]; nlen = (int)run.run_length; nop = run.op; }
            unsigned ti, tj;
            const unsigned i0 = ci + sum_wave_scan(op != GNX_COL_I ? (unsigned)len : 0u, lane, ti);
            const unsigned j0 = cj + sum_wave_scan(op != GNX_COL_D ? (unsigned)len : 0u, lane, tj);
            const unsigned long long nz = __ballot(len > 0);
            const unsigned long long nzb = nz & below;
            int pop = __shfl(op, nzb ? 63 - __clzll((long long)nzb) : 0, 64); // the seam rule: the op of the column before this run
            if (!nzb) pop = seg_op;
            const bool head = len > 0 && pop != op;
            const unsigned long long hm = __ballot(head), hb = hm & below;
            // the segment this head closes: from the head before it, or the carried one
            const int hl = hb ? 63 - __clzll((long long)hb) : 0;
            unsigned pi = __shfl(i0, hl, 64), pj = __shfl(j0, hl, 64);
            if (!hb) { pi = seg_i; pj = seg_j; }
            int kind = 0;
            unsigned long long key = 0;
            int64_t x = 0;
            if (head && pop == GNX_COL_D && pi >= a_start && pi < a_end) {
                kind = 1; key = i0 - pi; x = x0 + pi;
            } else if (head && pop == GNX_COL_I && pi > a_start && pi < a_end) {
                const unsigned L = j0 - pj;
                x = x0 + pi - 1;
                if (L > (unsigned)PILE_SEQ_MAX) { kind = 3; key = L; }
                else {
                    kind = 2;
                    for (unsigned k = 0; k < L; k++) key |= (unsigned long long)(min((int)rd[pj + k], 4) + 1) << (3 * k); // (a byte >= 5 fails the call before this kernel runs)
                }
            }
            const bool ev = kind != 0 && x >= 0 && x < a.region_len;
            const unsigned long long em = __ballot(ev);
            if (em) {
                unsigned long long base = 0;
                if (lane == __ffsll((long long)em) - 1) base = atomicAdd(a.cursor, (unsigned long long)__popcll(em));
                base = __shfl(base, __ffsll((long long)em) - 1, 64);
                const unsigned long long slot = base + __popcll(em & below);
                if (ev && slot < a.cap) { a.w0[slot] = (unsigned long long)x << 2 | (unsigned)kind; a.w1[slot] = key << 1 | sg; }
            }
            ci += ti; cj += tj;
            if (hm) { const int h = 63 - __clzll((long long)hm); seg_op = __shfl(op, h, 64); seg_i = __shfl(i0, h, 64); seg_j = __shfl(j0, h, 64); }
        }
    }
}

struct PileReduceArgs {
    const unsigned long long *w0, *w1; // sorted by (w0, w1)
    int64_t n, n_tiles;
    int64_t region_start;
    int64_t *cnt;       // WRITE = false: the group heads of each tile
    const int64_t *off; // WRITE = true: first slot of each tile
    gnx_pile_allele *out;
};

// the first entry in (lo, n) that is greater than (k0, k1) in the order of the sorted log; entry lo is not greater
__device__ __forceinline__ int64_t pile_upper(const PileReduceArgs &a, int64_t lo, unsigned long long k0, unsigned long long k1) {
    int64_t hi = a.n;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        const unsigned long long m0 = a.w0[mid];
        if (m0 > k0 || (m0 == k0 && a.w1[mid] > k1)) hi = mid; else lo = mid;
    }
    return hi;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void allele_reduce_kernel(PileReduceArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < a.n_tiles; t += (int64_t)gridDim.x * 4) {
        int64_t n_tile = WRITE ? a.off[t] : 0;
        for (int s = 0; s < PILE_TILE; s += 64) {
            const int64_t e = t * PILE_TILE + s + lane;
            if (t * PILE_TILE + s >= a.n) break;
            bool head = false;
            unsigned long long w0 = 0, w1 = 0;
            if (e < a.n) {
                w0 = a.w0[e]; w1 = a.w1[e];
                head = e == 0 || a.w0[e - 1] != w0 || (a.w1[e - 1] >> 1) != (w1 >> 1);
            }
            if (WRITE) {
                unsigned total;
                const int64_t slot = n_tile + sum_wave_scan(head ? 1u : 0u, lane, total);
                if (head) {
                    const int64_t end = pile_upper(a, e, w0, w1 | 1ull);
                    const int64_t fwd_end = (w1 & 1ull) ? e : pile_upper(a, e, w0, w1); // (a head on strand 1: no strand-0 entry)
                    const unsigned long long key = w1 >> 1;
                    gnx_pile_allele o;
                    o.pos = a.region_start + (int64_t)(w0 >> 2);
                    o.kind = (uint8_t)(w0 & 3ull); o._pad[0] = o._pad[1] = o._pad[2] = 0;
                    o.seq = o.kind == 2 ? key : 0ull;
                    o.length = o.kind == 2 ? (66 - __clzll((long long)key)) / 3 : (int32_t)key; // (the digits of a packed sequence: none is 0)
                    o.count = (int32_t)(end - e); o.count_fwd = (int32_t)(fwd_end - e);
                    a.out[slot] = o;
                }
                n_tile += total;
            } else n_tile += sum_wave_sum(head ? 1u : 0u);
        }
        if (!WRITE && lane == 0) a.cnt[t] = n_tile;
    }
}

struct PileIndelCallArgs {
    PileCallArgs c;               // the planes, the packed reference, the options; cnt / off per tile of alleles; c.out is not used
    const gnx_pile_allele *alleles;
    int64_t n;
    gnx_pile_indel_call *out;
};

template <bool WRITE>
__global__ __launch_bounds__(256) void allele_call_kernel(PileIndelCallArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < a.c.n_tiles; t += (int64_t)gridDim.x * 4) {
        int64_t n_tile = WRITE ? a.c.off[t] : 0;
        for (int s = 0; s < PILE_TILE; s += 64) {
            const int64_t e = t * PILE_TILE + s + lane;
            if (t * PILE_TILE + s >= a.n) break;
            bool pass = false;
            int depth = 0, c = 4;
            gnx_pile_allele al;
            if (e < a.n) {
                al = a.alleles[e];
                BetaSrcT<1> R;
                R.init(nullptr, a.c.kp, al.pos, 1);
                c = R.at(0);
                const int *q = a.c.pile + (al.pos - a.c.region_start);
                const int64_t L = a.c.region_len;
#pragma unroll
                for (int b = 0; b < 10; b++) depth += q[b * L];
                depth += q[PILE_DEL * L] + q[(PILE_DEL + 1) * L];
                pass = c < 4 && pile_passes(a.c, depth, al.count, al.count_fwd);
            }
            if (WRITE) {
                unsigned total;
                const int64_t slot = n_tile + sum_wave_scan(pass ? 1u : 0u, lane, total);
                if (pass) {
                    gnx_pile_indel_call o;
                    o.pos = al.pos; o.seq = al.seq; o.length = al.length; o.count = al.count; o.count_fwd = al.count_fwd;
                    o.kind = al.kind; o._pad[0] = o._pad[1] = o._pad[2] = 0;
                    o.depth = depth; o.ref = (uint8_t)c; o._pad2[0] = o._pad2[1] = o._pad2[2] = 0;
                    a.out[slot] = o;
                }
                n_tile += total;
            } else n_tile += sum_wave_sum(pass ? 1u : 0u);
        }
        if (!WRITE && lane == 0) a.c.cnt[t] = n_tile;
    }
}

} // namespace
