// pile_qual.hip.h -- base qualities in the pile and diploid SNP genotypes from them (contract: gnx_align.h)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit), behind pileup.hip.h.
//
// A pile that tracks qualities (gnx_pileup_track_qualities) has four more planes of region_len int32 beside the 14: qsum[A C G T], the
// summed Phred qualities of the counted read bases, both strands.  They are a buffer of their own, so every kernel of pileup.hip.h,
// pile_alleles.hip.h and pile_norm.hip.h indexes its planes as before and none of them changed.
//
// qual_add_kernel is pile_add_kernel with a quality byte read beside every read byte of an M column (a parallel array, same read_start):
// the same geometry -- one wave per pair, four per workgroup, the CIGAR in blocks of 64 runs loaded a block ahead, sum_wave_scan giving
// every run its origin, alpha_start / alpha_end taken before the walk, the same seam rule for I runs, both walking forms with the cut at
// 64 columns -- and the same adds for D columns and I runs, which have no quality.  An M column over read byte b with quality
// q = min(byte, 93): nothing if q < min_baseq; else base[strand][b] += 1 and, for b < 4 and q > 0, qsum[b] += q -- a second atomicAdd
// whose result is not used.  In the lane-per-column form both adds of a wave fall on 64 consecutive counters of their planes.  A read
// adds at most 93 to a qsum counter and the host keeps reads_added of a quality pile at or below (2^31 - 1) / 93: no counter overflows.
// pile_add_kernel itself is untouched (a plain pile launches what it launched before), which is why this is a kernel of its own and
// not a template over a shared body: the plain kernel's registers are pinned by tests/test_pileup_cpu.py.
//
// geno_call_kernel<WRITE> is pile_call_kernel's geometry -- one position per lane, PILE_TILE positions per wave in steps of 64, one
// coalesced read per plane (the 8 A C G T count planes and the 4 qsum planes), the reference code through BetaSrcT<1>, count / scan /
// write -- around geno_rule() (geno_rule.h), the per-position rule a CPU program can call as well.
#pragma once
#include "pileup.hip.h"
#include "geno_rule.h"

namespace {

constexpr int QUAL_PLANES = 4;  // qsum[A C G T]
constexpr int QUAL_MAX = 93;    // a quality byte above it counts as 93
constexpr int64_t QUAL_MAX_READS = (int64_t)INT32_MAX / QUAL_MAX; // 23 091 222

struct QualAddArgs {
    PileArgs p;
    const uint8_t *quals; // laid out like p.reads: raw Phred, the orientation of the read
    int *qsum;            // QUAL_PLANES planes of region_len sums
    int min_baseq;
};

// an inside M column at alpha position i over read byte rb with quality byte qb
__device__ __forceinline__ void qual_bump(const PileWin &w, int *qsum, int min_baseq, int sb, int rb, int qb, int i) {
    const int q = min(qb, QUAL_MAX), b = min(rb, 4);
    if (q < min_baseq || i < w.lo || i >= w.hi) return;
    const int64_t x = w.x0 + i;
    (void)atomicAdd(w.pile + ((int64_t)(sb + b) * w.len + x), 1);
    if (b < 4 && q > 0) (void)atomicAdd(qsum + ((int64_t)b * w.len + x), q);
}

__global__ __launch_bounds__(256) void qual_add_kernel(QualAddArgs qa) {
    const PileArgs &a = qa.p;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += (int64_t)gridDim.x * 4) {
        if (a.use && !a.use[p]) continue;
        const int64_t r0 = a.ops_off[p], nr = a.ops_off[p + 1] - r0;
        const int64_t rs = a.read_start[p];
        const uint8_t *rd = a.reads + rs, *qd = qa.quals + rs;
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
                if (mrun) for (int k = 0; k < len; k++) qual_bump(w, qa.qsum, qa.min_baseq, sb, rd[j0 + k], qd[j0 + k], i0 + k); // (a byte >= 5 fails the call before this kernel runs)
                else for (int k = 0; k < len; k++) pile_bump(w, PILE_DEL + sg, i0 + k);
            }
            for (unsigned long long cm = __ballot(coop); cm; cm &= cm - 1) { // lane per column
                const int o = __ffsll((long long)cm) - 1;
                const int ui0 = __shfl(i0, o, 64), uj0 = __shfl(j0, o, 64), ulen = __shfl(len, o, 64);
                if (__shfl(op, o, 64) == GNX_COL_M) for (int k = lane; k < ulen; k += 64) qual_bump(w, qa.qsum, qa.min_baseq, sb, rd[uj0 + k], qd[uj0 + k], ui0 + k);
                else for (int k = lane; k < ulen; k += 64) pile_bump(w, PILE_DEL + sg, ui0 + k);
            }
            ci += ti; cj += tj;
            if (nz) prev_op = __shfl(op, 63 - __clzll((long long)nz), 64);
        }
    }
}

struct GenoCallArgs {
    KParams kp;        // only the packed-reference pointers are read
    const int *pile;   // the 14 planes
    const int *qsum;   // the 4 quality planes
    int64_t region_start, region_len, n_tiles;
    GenoOpts o;
    int64_t *cnt;       // WRITE = false: the records of each tile, contiguous for the scan
    const int64_t *off; // WRITE = true: first slot of each tile
    gnx_pile_genotype *out;
};

template <bool WRITE>
__global__ __launch_bounds__(256) void geno_call_kernel(GenoCallArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < a.n_tiles; t += (int64_t)gridDim.x * 4) {
        int64_t n_tile = WRITE ? a.off[t] : 0; // records of the tile so far (WRITE: on top of its first slot)
        for (int s = 0; s < PILE_TILE; s += 64) {
            const int64_t r = t * PILE_TILE + s; // the step's first position in the region
            if (r >= a.region_len) break;
            const int nv = a.region_len - r < 64 ? (int)(a.region_len - r) : 64;
            BetaSrcT<1> R;
            R.init(nullptr, a.kp, a.region_start + r, nv);
            GenoRec rec;
            bool hit = false;
            int c = 4;
            if (lane < nv) {
                c = R.at(lane);
                const int64_t L = a.region_len;
                const int *q = a.pile + (r + lane), *qs = a.qsum + (r + lane);
                int32_t fwd[4], rev[4], sum[4];
#pragma unroll
                for (int b = 0; b < 4; b++) { fwd[b] = q[b * L]; rev[b] = q[(5 + b) * L]; sum[b] = qs[b * L]; }
                hit = geno_rule(fwd, rev, sum, c, a.o, rec);
            }
            if (WRITE) {
                unsigned total;
                const int64_t slot = n_tile + sum_wave_scan(hit ? 1u : 0u, lane, total);
                if (hit) {
                    gnx_pile_genotype g;
                    g.pos = a.region_start + r + lane;
                    g.pl[0] = rec.pl[0]; g.pl[1] = rec.pl[1]; g.pl[2] = rec.pl[2];
                    g.gq = rec.gq; g.qual = rec.qual; g.depth = rec.depth; g.ref_count = rec.ref_count; g.alt_count = rec.alt_count; g.alt_fwd = rec.alt_fwd;
                    g.gt = (uint8_t)rec.gt; g.ref = (uint8_t)c; g.alt = (uint8_t)rec.alt; g._pad = 0;
                    a.out[slot] = g;
                }
                n_tile += total;
            } else n_tile += sum_wave_sum(hit ? 1u : 0u);
        }
        if (!WRITE && lane == 0) a.cnt[t] = n_tile;
    }
}

} // namespace
