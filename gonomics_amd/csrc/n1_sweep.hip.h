// n1_sweep.hip.h -- score-only sweep with explicit cell scores: what gnx_affine_gap_chunk_score_batch / gnx_multiple_affine_gap_score_batch run
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.17.
#pragma once
#include "score_sweep.hip.h"

namespace {
// ------------------------------------------------------------------------------------------------------
// The global affine score sweep of score_sweep.hip.h (section 4.15) for the chunk / multiple-alignment variants, whose cell score is
// not a function of two bases: the diagonal term of cell (row, column) comes from a per-pair device matrix instead of the LDS profile.
// The body is score_sweep_body with MatrixSource, the levels loop is sweep_levels: 16 lanes x 10 rows, a quad of four pairs per wave,
// rows right-aligned over the levels, plain keys rebased by (row + column), the cell  add, max3, add, max, max,  the hand-over of the
// bottom row between levels (rb_store / rb_publish / rb_progress, claim_items, the bounded wait that raises err bit 16 and the
// level-by-level fallback) are there.  This file holds what is the matrix's own.
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

struct N1Plan {
    int32_t n, m;       // rows (the side held in lanes, the shorter one) and columns, in chunk cells; n == 0: an empty slot of the last quad
    int32_t src;        // index of the pair in the score vector
    int32_t levels;     // S of the pair's quad
    int64_t rowbuf_off; // int2: the pair's two hand-over rows of m + 1 entries (pairs of more than one level)
    int64_t mat_off;    // int16: the pair's matrix (first pad entry of column 1)
    int32_t pitch;      // int16 entries per column: n + pad
    int32_t _pad;
};

// the source of score_sweep_body's diagonal term (score_sweep.hip.h): the matrix, read through a register ring of N1_D column loads
struct MatrixSource {
    static constexpr bool MATRIX = true;
    static constexpr int LINK = 0, D = N1_D;
    const short *mat;
};

// pairs of one row block (the shorter side <= 160 chunk cells): one wave per quad
__global__ __launch_bounds__(64) void n1_sweep_kernel(const N1Plan *__restrict__ plans, const short *__restrict__ mat, int o, int e,
                                                      int64_t *__restrict__ out_score, int *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) int lds[N1_LDS];
    score_sweep_body<SS_RR, true>(lds, (int)blockIdx.x, plans, MatrixSource{mat}, o, e, out_score, err, nullptr, 0, false, false, false, nullptr, nullptr);
}

// quads of S >= 2 row blocks: grid, claims and arguments as sweep_levels (score_sweep.hip.h) says
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
    // nothing goes into LDS up front, and there are no packed-reference pointers to read per level: the first two callables are
    // empty (sweep_levels keeps the slot of `kparams` in front of its barrier, where the profile kernels had that read)
    sweep_levels<N1LevelsArgs>([](auto) {}, [](auto) { return 0; }, [&](auto ka, int, int w, int level, bool takes, bool hands, const int *pi, int *po) {
        score_sweep_body<SS_RR, true>(lds, w, ka->plans, MatrixSource{ka->mat}, ka->o, ka->e, ka->out_score, ka->err, ka->rowbuf, level, takes, hands, ka->piped != 0, pi, po);
    });
}

} // namespace
