// n1_sweep.hip.h -- score-only sweep with explicit cell scores: what gnx_affine_gap_chunk_score_batch / gnx_multiple_affine_gap_score_batch run
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.17.
#pragma once
#include "score_sweep.hip.h"

namespace {
// ------------------------------------------------------------------------------------------------------
// The global affine score sweep of score_sweep.hip.h (section 4.15) for the chunk / multiple-alignment variants, whose cell score is
// not a function of two bases: the diagonal term of cell (row, column) comes from a per-pair device matrix instead of the LDS profile.
// Unchanged: 16 lanes x 10 rows, a quad of four pairs per wave, rows right-aligned over the levels, plain keys rebased by (row +
// column), the cell  add, max3, add, max, max,  the hand-over of the bottom row between levels (rb_store / rb_publish / rb_progress,
// claim_items, the bounded wait that raises err bit 16 and the level-by-level fallback).
// The matrix (written by the SWP instantiations of the score-matrix kernels, aux_kernels.hip.h): int16 entries s - 2e, column-major,
//   column c of a pair = [pad entries of -32768][the n entries of rows 1 .. n],  pad = (10 - n % 10) % 10,  pitch = n + pad
// so that the rows are right-aligned to a LANE: a lane's ten entries of a column are 20 contiguous bytes that start on a dword
// (pitch and every lane offset are even), the lane that holds padding and real rows together reads its "never wins" entries from the
// matrix itself, and nobody reads outside a column.  Lanes made of padding alone (and the empty slots of the last quad) read a block
// of -32768 entries at the head of the buffer with stride 0; the layout does not depend on the number of levels of the pair's quad.
// A lane is at column t - lp at step t; its entries are loaded N1_D steps ahead of their use into a register ring (one dwordx4 + one
// dword load per step and wave).  Columns outside 1 .. m are clamped into the matrix: those cells are not live.
// No LDS profile, no base rings, no bases: LDS holds the hand-over ring and the staging of the row handed down only.
// ------------------------------------------------------------------------------------------------------
constexpr int N1_D = 4;                                   // steps between a load and its use
constexpr int N1_LDS = 4 * SS_RING * 2 + 4 * 16 * 2;      // dwords per wave: hand-over ring, staging of the row handed down
constexpr int N1_PADBLOCK = 32;                           // int16 entries of -32768 at the head of the matrix buffer
static_assert(16 % N1_D == 0, "the ring slot of a step is its position in a chunk of 16");

struct N1Plan {
    int32_t n, m;       // rows (the side held in lanes, the shorter one) and columns, in chunk cells; n == 0: an empty slot of the last quad
    int32_t src;        // index of the pair in the score vector
    int32_t levels;     // S of the pair's quad
    int64_t rowbuf_off; // int2: the pair's two hand-over rows of m + 1 entries (pairs of more than one level)
    int64_t mat_off;    // int16: the pair's matrix (first pad entry of column 1)
    int32_t pitch;      // int16 entries per column: n + pad
    int32_t _pad;
};

typedef int n1_int4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void n1_sweep_body(int *__restrict__ lds, const int quad, const N1Plan *__restrict__ plans, const short *__restrict__ mat,
                                              const int sp_o, const int sp_e, int64_t *__restrict__ out_score, int *__restrict__ err,
                                              int2 *__restrict__ rowbuf, const int level, const bool TAKES, const bool HANDS, const bool piped, const int *prog_in, int *prog_out) {
    constexpr int RR = SS_RR, HB = G * RR, NW = RR / 2;
    const int lane = threadIdx.x;
    const int g = lane >> 4, lp = lane & 15;
    const int O = sp_o;
    int2 *hring = reinterpret_cast<int2 *>(lds) + g * SS_RING;              // [column & 31] = {D'(first row, column), h'(row above, column)}
    int2 *hand = reinterpret_cast<int2 *>(lds + 4 * SS_RING * 2) + g * 16;

    int m_max = 0, m_min = 0x7fffffff;
    for (int q = 0; q < 4; q++) {
        const N1Plan &pq = plans[quad * 4 + q];
        if (pq.n > 0) { m_max = max(m_max, pq.m); m_min = min(m_min, pq.m); }
    }
    const N1Plan pl = plans[quad * 4 + g];
    const bool valid = pl.n > 0;
    const int m_eff = valid ? pl.m : 0;
    const int P = pl.levels * HB - pl.n;          // padding slots above row 1 (over all levels of the pair)
    const int q0 = level * HB + lp * RR;          // first slot of this lane; slot q holds row q - P + 1 of the pair
    const int P10 = P - P % RR;                   // first slot of the lane that holds row 1: the matrix columns start there
    const bool live = valid && q0 >= P10;         // this lane reads the matrix (else: the block of padding entries, stride 0)
    const char *cbase = reinterpret_cast<const char *>(live ? mat + pl.mat_off + (q0 - P10) : mat);
    const unsigned cstride = live ? (unsigned)pl.pitch * 2u : 0u;
    const int m_c = max(m_eff, 1);
    auto load_col = [&](int j, int *w) { // this lane's RR entries of column j
        const unsigned idx = (unsigned)(min(max(j, 1), m_c) - 1);
        const char *p = cbase + (unsigned long long)idx * cstride;
        const n1_int4 v = *reinterpret_cast<const n1_int4 *>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        w[4] = *reinterpret_cast<const int *>(p + 16);
    };
    static_assert(NW == 5, "a lane's entries are one 16-byte and one 4-byte load");

    // column 0 (score_sweep.hip.h): real row: h' = D' = o, I'(i,1) = 2o; padding: h' = I' = o; the slot above row 1: h'(0,0) = 0
    auto hcol0 = [&](int q) { return q != P - 1 ? O : 0; };
    int rt[RR], hold[RR];
#pragma unroll
    for (int r = 0; r < RR; r++) {
        hold[r] = hcol0(q0 + r);
        rt[r] = (q0 + r >= P) ? 2 * O : O;
    }
    int diag0 = hcol0(q0 - 1);
    int dn_out = 0, h_out = 0;
    int up_dn = 2 * O, up_h = O; // level 0: the first lane keeps the row-0 constants as the `old` operand of its DPP moves
    int vO;
    asm volatile("v_mov_b32 %0, %1" : "=v"(vO) : "s"(O));

    const int2 *rb_in = (TAKES && valid) ? rowbuf + pl.rowbuf_off + (int64_t)((level - 1) & 1) * (pl.m + 1) : nullptr;
    int2 *rb_out = (HANDS && valid) ? rowbuf + pl.rowbuf_off + (int64_t)(level & 1) * (pl.m + 1) : nullptr;
    int rb_seen = 0;
    // piped: wait until the level above has handed down the columns <= c (it stores column c after its step c + 15)
    auto wait_cols = [&](int c) {
        if (TAKES && piped && rb_seen < c + G - 1) {
            const long long t_begin = wall_clock64();
            while ((rb_seen = rb_progress(prog_in)) < c + G - 1) {
                __builtin_amdgcn_s_sleep(32);
                if (wall_clock64() - t_begin > 500000000LL) { atomicOr(err, 16); break; } // 5 s at 100 MHz
            }
        }
    };
    auto rb_at = [&](int c) { return (TAKES && c >= 1 && c <= m_eff) ? rb_load(&rb_in[c], piped) : make_int2(0, 0); };
    // prologue: the hand-over of columns 0 .. 31 into the ring, the loads of columns 32 .. 47 in flight
    int2 rqn = make_int2(0, 0);
    if (TAKES) {
        wait_cols(min(m_max, 47));
        hring[lp] = rb_at(lp);
        hring[16 + lp] = rb_at(16 + lp);
        rqn = rb_at(32 + lp);
        __syncthreads();
    }
    int ring[N1_D][NW]; // slot s: the entries of the step at position s (mod N1_D) of a chunk
#pragma unroll
    for (int s = 0; s < N1_D; s++) load_col(s - lp, ring[s]);
    int2 rq = TAKES ? hring[0] : make_int2(0, 0), rq1 = TAKES ? hring[1] : make_int2(0, 0); // what the first lane takes at steps 0 and 1

    auto step = [&](const int t, const int slot, auto chk) {
        constexpr bool CHECK = decltype(chk)::value; // false: every lane of the wave is inside its matrix
        up_dn = dpp_shr1(TAKES ? rq.x : up_dn, dn_out);
        up_h = dpp_shr1(TAKES ? rq.y : up_h, h_out);
        if (TAKES) { rq = rq1; rq1 = hring[(t + 2) & (SS_RING - 1)]; }
        int wq[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) wq[k] = ring[slot][k];
        load_col(t + N1_D - lp, ring[slot]); // this slot's next use is N1_D steps away
        asm volatile("" ::: "memory");       // the loads stay HERE, ahead of the arithmetic
        const int j = t - lp;
        if (!CHECK || (j >= 1 && j <= m_eff)) {
            int hd = diag0, dnu = up_dn;
#pragma unroll
            for (int r = 0; r < RR; r++) {
                const int S = (r & 1) ? (wq[r >> 1] >> 16) : (int)(short)(wq[r >> 1] & 0xffff);
                const int M = hd + S;
                hd = hold[r];
                const int hnew = max3i(M, rt[r], dnu);
                const int ho = hnew + vO;
                rt[r] = max(ho, rt[r]);
                dnu = max(ho, dnu);
                hold[r] = hnew;
            }
            diag0 = up_h;
            dn_out = dnu;
            h_out = hold[RR - 1];
            if (HANDS) { if (lp == G - 1) hand[t & 15] = make_int2(dn_out, h_out); }
        }
    };
    auto chunk_head = [&](int t0) { // hand-over ring: columns t0 + 16 .. t0 + 31 from the loads of the chunk before; loads of t0 + 32 .. t0 + 47
        if (TAKES) {
            hring[(t0 + 16 + lp) & (SS_RING - 1)] = rqn;
            wait_cols(min(m_max, t0 + 47));
            rqn = rb_at(t0 + 32 + lp);
            __syncthreads();
        }
    };
    auto hand_down = [&](int t0) { // after the steps t0 .. t0 + 15: the last lane was at the columns t0 - 15 .. t0
        if (HANDS) {
            __syncthreads();
            const int c = t0 - (G - 1) + lp;
            const int2 v = hand[lp];
            if (valid && c >= 1 && c <= m_eff) rb_store(&rb_out[c], v.x, v.y, piped);
            __syncthreads();
            if (piped && ((t0 + 16) & (GNX_SS_PUB - 1)) == 0) rb_publish(prog_out, t0 + 15, lane);
        }
    };
    // chunks of 16 steps; the steady ones (every lane of the wave inside its matrix) run without the per-lane test
    const int Tend = ((m_max + G - 1) / 16 + 1) * 16;
    for (int t0 = 0; t0 < Tend; t0 += 16) {
        if (t0 > 0) chunk_head(t0);
        if (t0 >= 16 && t0 + 15 <= m_min) {
#pragma unroll
            for (int u = 0; u < 16; u++) step(t0 + u, u & (N1_D - 1), std::false_type{});
        } else {
#pragma unroll 1
            for (int u0 = 0; u0 < 16; u0 += N1_D) {
#pragma unroll
                for (int s = 0; s < N1_D; s++) step(t0 + u0 + s, s, std::true_type{});
            }
        }
        hand_down(t0);
    }
    if (HANDS && piped) rb_publish(prog_out, 0x7fffffff, lane);
    if (!HANDS && lp == G - 1 && valid) out_score[pl.src] = (int64_t)hold[RR - 1] + (int64_t)sp_e * ((int64_t)pl.n + pl.m);
}

// pairs of one row block (the shorter side <= 160 chunk cells): one wave per quad
__global__ __launch_bounds__(64) void n1_sweep_kernel(const N1Plan *__restrict__ plans, const short *__restrict__ mat, int o, int e,
                                                      int64_t *__restrict__ out_score, int *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) int lds[N1_LDS];
    n1_sweep_body(lds, (int)blockIdx.x, plans, mat, o, e, out_score, err, nullptr, 0, false, false, false, nullptr, nullptr);
}

// quads of S >= 2 row blocks: grid, claims and arguments as in score_sweep_levels_kernel
struct N1LevelsArgs {
    const N1Plan *plans; const short *mat;
    int o, e;
    int64_t *out_score; int *err; int2 *rowbuf;
    int S, W, level0, piped;
    int *prog;
};
__global__ __launch_bounds__(64) void n1_sweep_levels_kernel(N1LevelsArgs by_value) {
    __shared__ __attribute__((aligned(16))) int lds[N1_LDS];
    (void)by_value;
    typedef const __attribute__((address_space(4))) N1LevelsArgs *ArgPtr;
    ArgPtr ka = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const int W = ka->W;
    const int lv_own = (int)blockIdx.x / W, w = (int)blockIdx.x - lv_own * W;
    int n_stolen = 0;
    if (ka->piped) { n_stolen = claim_items(ka->prog + (int64_t)ka->S * W, W, lv_own); if (n_stolen < 0) return; }
    for (int lv = lv_own - n_stolen; lv <= lv_own; lv++) {
        asm volatile("" : "+s"(ka));
        const int S = ka->S, Wk = ka->W, level = ka->level0 + lv;
        int *po = ka->prog + (int64_t)level * Wk + w;
        const int *pi = po - Wk;
        if (lv != lv_own - n_stolen) __syncthreads(); // the LDS rings of the level before are no longer read
        n1_sweep_body(lds, w, ka->plans, ka->mat, ka->o, ka->e, ka->out_score, ka->err, ka->rowbuf, level, level > 0, level < S - 1, ka->piped != 0, pi, po);
    }
}

} // namespace
