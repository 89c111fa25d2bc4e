// pile_norm.hip.h -- the pile's indel alleles left-normalised against the resident reference (contract: gnx_align.h)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit) beside pile_alleles.hip.h.
//
// norm_shift_kernel reads the two planes of a tracking pile's log and writes every event, moved to the leftmost placement the reference
// admits inside the region, into two scratch planes of the same layout; the log stays raw.  gnx_pileup_alleles_norm then runs the plain
// query's two sorts over the scratch planes, and the reduce and the call kernels see a log like any other.
//
// The rule (gnx_align.h) in the form the kernel uses: an allele of length L at region offset xr moves by d = the run of positions
// y = y0, y0 - 1, ... with T[y] == T[y + L], both A C G T, at most xr of them.  A deletion has T = the reference and y0 = x - 1.  An
// insertion behind x has T = the reference up to x followed by its own bases, y0 = x: its first min(d, L) comparisons are against its own
// bases from the last one down (norm_ins_head: a loop of at most 21 steps), and once they all hold it is the reference against itself at
// distance L from y = x - L on, as for a deletion.  The moved insertion's bases are its own, rotated by d mod L (norm_key_rotate): no
// reference read rebuilds them.  A longer insertion (kind 3) kept no bases and stays where it is.
//
// Geometry, one lane per event of a wave's 64, in two phases:
//   1  every lane compares NORM_LANE_CHUNKS chunks of 32 bases of its own (norm_chunk_run: two 64-bit values cut out of the packed dwords, an
//      XOR and a leading-zero count; base by base through BetaSrcT<1>::at where a chunk touches a flagged 64-base block or the region's start).
//   2  the events whose run has not ended are found by a ballot and taken one after the other by the whole wave: lane l compares the
//      chunk 32 * l bases further left, 2 048 bases a step, and the first lane (a ballot again) whose run is short closes the total.
//      A satellite array of thousands of exact repeat units costs a few steps of one wave, not hundreds of chunk steps of one lane that
//      holds its 63 neighbours.  GNX_NORM_COOP=0 (`coop` 0) lets every lane finish alone instead; the counts are integers and do not depend
//      on who took them.
// Nothing is read below the region's start (rem counts the steps it admits) or behind the allele's own last base.  No LDS, no scratch.
#pragma once
#include "pile_alleles.hip.h"
#include "norm_shift.h"

namespace {

constexpr int NORM_LANE_CHUNKS = 1; // chunks a lane compares alone before the wave takes its event over

struct NormArgs {
    KParams kp;                         // only the packed-reference pointers are read
    const unsigned long long *w0, *w1;  // the log's planes
    unsigned long long *o0, *o1;        // the normalised events, in the log's order
    int64_t n;
    int64_t region_start, ref_len;
    int coop;
};

__global__ __launch_bounds__(256) void norm_shift_kernel(NormArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned *b2 = a.kp.b2;
    const unsigned long long *bflag = a.kp.bflag;
    auto at = [&](int64_t x) -> int {
        BetaSrcT<1> R;
        R.init(nullptr, a.kp, x, 1);
        return R.at(0);
    };
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t e0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; e0 < a.n; e0 += n_waves * 64) {
        const int64_t e = e0 + lane;
        unsigned long long w0 = 0, w1 = 0;
        int kind = 0;
        if (e < a.n) { w0 = a.w0[e]; w1 = a.w1[e]; kind = (int)(w0 & 3ull); }
        const int64_t xr = (int64_t)(w0 >> 2), x = a.region_start + xr;
        const unsigned long long key = w1 >> 1;
        int64_t L = 0, y = 0, rem = 0, d = 0; // rem: the steps left to the region's start; y: the next comparison
        if (kind == 1) { L = (int64_t)key; y = x - 1; rem = xr; }
        else if (kind == 2) {
            L = norm_key_len(key);
            d = norm_ins_head(at, key, (int)L, x, xr);
            if (d == L) { y = x - L; rem = xr - L; }
        }
        if (L <= 0 || L > a.ref_len - 1 - y) rem = 0; // (no base behind the reference is ever compared)
        bool open = rem > 0;
        for (int c = 0; c < NORM_LANE_CHUNKS; c++) {
            if (open) {
                const int r = norm_chunk_run(b2, bflag, at, y, L, rem);
                d += r; y -= r; rem -= r;
                open = r == NORM_CHUNK && rem > 0;
            }
        }
        if (a.coop) {
            for (unsigned long long om = __ballot(open); om; om &= om - 1) {
                const int o = __ffsll((long long)om) - 1;
                const int64_t uL = __shfl(L, o, 64);
                int64_t uy = __shfl(y, o, 64), urem = __shfl(rem, o, 64), tot = 0;
                for (;;) {
                    const int64_t my = urem - (int64_t)NORM_CHUNK * lane;
                    const int r = my > 0 ? norm_chunk_run(b2, bflag, at, uy - (int64_t)NORM_CHUNK * lane, uL, my) : 0;
                    const unsigned long long sm = __ballot(r < NORM_CHUNK);
                    if (sm) {
                        const int f = __ffsll((long long)sm) - 1;
                        tot += (int64_t)NORM_CHUNK * f + __shfl(r, f, 64);
                        break;
                    }
                    tot += 64 * NORM_CHUNK; uy -= 64 * NORM_CHUNK; urem -= 64 * NORM_CHUNK;
                }
                if (lane == o) d += tot;
            }
        } else {
            while (open) {
                const int r = norm_chunk_run(b2, bflag, at, y, L, rem);
                d += r; y -= r; rem -= r;
                open = r == NORM_CHUNK && rem > 0;
            }
        }
        if (e < a.n) {
            a.o0[e] = (unsigned long long)(xr - d) << 2 | (unsigned)kind;
            a.o1[e] = kind == 2 ? norm_key_rotate(key, (int)L, d) << 1 | (w1 & 1ull) : w1;
        }
    }
}

} // namespace
