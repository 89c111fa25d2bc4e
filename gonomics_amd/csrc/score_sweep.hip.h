// score_sweep.hip.h -- score-only sweep (16 lanes x RR rows per pair, plain rebased keys): what the gnx_score_* entries run
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.15.
#pragma once
#include "gnx_common.hip.h"

namespace {
// ------------------------------------------------------------------------------------------------------
// The global score h(n, m) of AffineGap* / ConstGap* without anything a CIGAR needs.  Same anti-diagonal wavefront as the other sweeps
// (lane lp of a pair holds RR consecutive rows and is at column t - lp at step t), re-cut for the case that keeps no route:
//  * keys are PLAIN scores (no tag bits, nothing scaled by 4), rebased like the fast path's: V' = V - e * (i + j) for the affine
//    planes, so that the cell is  add, max3, add, max, max  on every row
//        M' = h'(i-1,j-1) + (s - 2e)    h' = max3(M', I', D')    I'(i,j+1) = max(h' + o, I')    D'(i+1,j) = max(h' + o, D')
//    (needs gapOpen <= 0), and V' = V - g * (i + j) for the constant gap, whose two gap moves then cost nothing:
//        h'(i,j) = max3(h'(i-1,j-1) + (s - 2g), h'(i,j-1), h'(i-1,j))                                 -- add, max3.
//  * a global score does not change when the two sequences swap (with the transposed matrix), so the SHORTER sequence of every pair
//    is the one held in lanes (ScorePlan::swap, decided per pair by the host); the longer one streams by as columns.
//  * rows are RIGHT-ALIGNED over the S row blocks ("levels") of the pair's quad: the first P = S * 16 * RR - n slots are padding that
//    reproduces row 0 (profile entry -32768 so that M' never wins; affine: I' = h' = o, D' = 2o are fixed points when o <= 0, the slot
//    right above row 1 starts with h'(0,0) = 0; constant gap: everything 0).  Pairs of any length mix in one wave, a block made of
//    padding alone hands row 0 down unchanged, and h(n, m) always ends in the last slot of the last lane of the last level.
//  * one pair per 16-lane DPP row, four pairs (a QUAD) per wave: "value of the previous lane" is one row_shr:1 whose `old` operand
//    feeds the first lane -- the row-0 constants on level 0, the row the level above handed down otherwise.
//  * int16 profile (s - 2e per row and column base) in LDS, read one step ahead of its use as two ds_read_b64 + one ds_read_b32; a
//    lane's RR / 2 words sit in SS_LW = 6 dwords, so the 16 lanes of a pair start in 16 different even banks: conflict-free
//    whatever the bases are (planes are 64 * 6 dwords = 0 mod 32 apart).
//  * the column bases (as byte offsets of their profile plane) and the handed-down row reach the first lane through two small LDS
//    rings of 32 columns that the pair's lanes fill 16 columns at a time from loads issued a whole chunk earlier; from the first lane
//    the base travels down the lanes with the DP values (three DPP moves per step, two for the constant gap).
// No checkpoints, planes, events, snapshots or direction bits: global traffic is the bases, 16 bytes per column and level boundary
// (two rows of m + 1 entries per pair of more than one level, whatever the number of levels: level L writes row L & 1 behind the
// reader of the level above it), and 8 bytes of score per pair.
// Levels of a quad run as ONE launch (the levels kernels: sweep_levels), level-major like fp_sweep_levels_kernel, each level following
// the one above it through the row buffer with the same protocol (rb_store / rb_publish / rb_progress, claim_items for forward progress
// without any assumption about dispatch order, a bounded wait that raises err bit 16).
// ------------------------------------------------------------------------------------------------------
constexpr int SS_RR = 10;                 // rows per lane of the geometry that is built (a template parameter of the body)
constexpr int SS_LW = 6;                  // dwords per lane and plane (RR / 2 used)
constexpr int SS_PLANE = 64 * SS_LW;      // dwords per base plane
constexpr int SS_RING = 32;               // columns held by the base ring and the hand-over ring of a pair
constexpr int SS_LDS = 32 + 5 * SS_PLANE + 4 * SS_RING + 4 * SS_RING * 2 + 4 * 16 * 2; // dwords per wave: score table, profile, rings, staging of the row handed down
constexpr int SS_MAX_LEVELS = 64;         // row blocks per pair: the shorter sequence up to 64 * 160 = 10 240 bases
#ifndef GNX_SS_PUB
#define GNX_SS_PUB 64
#endif

struct ScorePlan {
    int32_t n, m;       // rows (the shorter sequence) and columns; n == 0: an empty slot of the last quad
    int32_t src;        // index of the pair in the start tables and in the score vector
    int32_t swap;       // 1: rows = beta, columns = alpha (and the matrix transposed)
    int64_t rowbuf_off; // int2: the pair's two hand-over rows of m + 1 entries (pairs of more than one level)
    int32_t levels;     // S of the pair's quad
    int32_t _pad;
};

struct ScoreParams {
    int sc[25]; // scores[a * 5 + b] - 2 * (affine: gapExtend; constant gap: gapPen)
    int o;      // affine: gapOpen
    int e;      // what the keys are rebased with: gapExtend / gapPen
};

// lds[0 .. 31]: the score table and the entry the padding rows read (sp: a pointer to the ScoreParams, in any address space)
//   global: -32768, the diagonal candidate never wins;  LOCAL: -2e, a diagonal move of score 0
template <bool LOCAL = false, class SpPtr>
__device__ __forceinline__ void score_table_to_lds(int *lds, SpPtr sp) {
    const int lane = threadIdx.x;
    if (lane < 25) lds[lane] = sp->sc[lane];
    else if (lane < 32) lds[lane] = LOCAL ? -2 * sp->e : -32768;
}

// what only the LOCAL body carries (an empty struct otherwise: the global instantiations hold nothing of it)
template <bool LOCAL> struct SweepLocal {};
template <> struct SweepLocal<true> {
    int zrow;   // level 0: the slot above the first one holds h = 0 at every column: h'(c) = -e * (c - P), stepped along with t (the first lane is at column t)
    int bshift; // the last row's running maximum of max(M, I) in the frame of the NEXT column (minus e per step); column 0 is I(0, n) = o + n * e
    int end_t;  // the step of its last >= update (the last lane is at column t - 15)
    int vE;     // gapExtend in a vector register (the levels kernel has no scalar register to spare)
};
// where a LOCAL body finds its two result vectors when it is done (the levels kernel reads them from its argument segment then)
struct NoOuts { __device__ __forceinline__ int64_t *score() const { return nullptr; } __device__ __forceinline__ int64_t *end() const { return nullptr; } };

typedef int ss_int4 __attribute__((ext_vector_type(4), aligned(4)));

// Where the diagonal term s - 2e of a cell comes from is the body's SOURCE, chosen at compile time.  A source holds what the body
// reads it from and says: MATRIX or not, the dwords of LDS in front of the level link (LINK: hring and hand), and the steps between
// a load and its use (D: the register ring slot of a step is its position mod D in a chunk of 16; 1: no register ring).
//   ProfileSource (here): the LDS profile of the lane's rows and the ring of column bases, filled from the two sequences.
//   MatrixSource (n1_sweep.hip.h): a per-pair device matrix, a lane's entries of a column loaded D steps ahead into registers.
// Everything else -- padding and column 0, the level link, the cell, the chunk driver, the write-back -- exists once.
struct ProfileSource {
    static constexpr bool MATRIX = false;
    static constexpr int LINK = 32 + 5 * SS_PLANE + 4 * SS_RING, D = 1;
    const uint8_t *a_buf; const int64_t *a_start; const uint8_t *b_buf; const int64_t *b_start; const KParams &kp;
};

// TAKES / HANDS: the block takes the row above it from the row buffer / hands its bottom row down (compile-time constants in the
// one-block kernels; wave-uniform run-time values in the levels kernels, which hold ONE copy of the body: three inlined copies leave
// them short of scalar registers)
template <int RR, bool AFF, bool LOCAL = false, class Plan, class Src, class Outs = NoOuts>
__device__ __forceinline__ void score_sweep_body(int *__restrict__ lds, const int quad, const Plan *__restrict__ plans, const Src &src,
                                                 const int sp_o, const int sp_e, int64_t *__restrict__ out_score, int *__restrict__ err,
                                                 int2 *__restrict__ rowbuf, const int level, const bool TAKES, const bool HANDS, const bool piped, const int *prog_in, int *prog_out,
                                                 const Outs outs = Outs()) {
    static_assert(RR == 2 * (SS_LW - 1), "profile words per lane");
    static_assert(AFF || !LOCAL, "the local sweep is affine");
    static_assert(16 % Src::D == 0, "the ring slot of a step is its position in a chunk of 16");
    constexpr bool MAT = Src::MATRIX;
    constexpr int HB = G * RR, NW = RR / 2; // rows of a block; dwords of a lane's entries of a column
    const int lane = threadIdx.x;
    const int g = lane >> 4, lp = lane & 15;
    const int O = AFF ? sp_o : 0;
    // State of ONE source is declared here for both, because the lambdas below capture it; the other source's stays unset and is
    // touched by nobody: its lambdas are called inside `if constexpr` branches of the source that owns them only.
    //   ProfileSource owns: prof, prof_lane, bring, cols, bad, nraw, pb, bnext, pbn, wn and col_raw / col_off / fetch
    //   MatrixSource owns:  cbase, cstride, m_c, ring and load_col
    // lds[0 .. 31]: the score table s - 2e and the padding entry, written by the kernel (score_table_to_lds)
    int *prof = lds + 32;
    const char *prof_lane = reinterpret_cast<const char *>(prof + lane * SS_LW);
    int *bring = prof + 5 * SS_PLANE + g * SS_RING;                                       // [column & 31] = byte offset of the column's profile plane
    int2 *hring = reinterpret_cast<int2 *>(lds + Src::LINK) + g * SS_RING; // [column & 31] = {D'(first row, column), h'(row above, column)}
    int2 *hand = reinterpret_cast<int2 *>(lds + Src::LINK + 4 * SS_RING * 2) + g * 16;

    int m_max = 0, m_min = 0x7fffffff;
    for (int q = 0; q < 4; q++) {
        const Plan &pq = plans[quad * 4 + q];
        if (pq.n > 0) { m_max = max(m_max, pq.m); m_min = min(m_min, pq.m); }
    }
    const Plan pl = plans[quad * 4 + g];
    const bool valid = pl.n > 0;
    const int m_eff = valid ? pl.m : 0;
    const int P = pl.levels * HB - pl.n;          // padding slots above row 1 (over all levels of the pair)
    const int q0 = level * HB + lp * RR;          // first slot of this lane; slot q holds row q - P + 1 of the pair
    // rows and columns: alpha is bytes, beta bytes or windows of the packed resident reference
    BetaSrc cols; // (ProfileSource)
    int bad = 0;
    // MATRIX: this lane's entries of a column are NW dwords at cbase + (column - 1) * cstride (n1_sweep.hip.h)
    const char *cbase;
    unsigned cstride;
    int m_c;
    if constexpr (MAT) {
        const int P10 = P - P % RR;                   // first slot of the lane that holds row 1: the matrix columns start there
        const bool live = valid && q0 >= P10;         // this lane reads the matrix (else: the block of padding entries, stride 0)
        cbase = reinterpret_cast<const char *>(live ? src.mat + pl.mat_off + (q0 - P10) : src.mat);
        cstride = live ? (unsigned)pl.pitch * 2u : 0u;
        m_c = max(m_eff, 1);
    } else { // int16 profile of this lane's rows: prof[b][lane][r] = scores[row base][b] - 2e (swap: scores[b][row base]), padding -32768
        BetaSrc sa, sb, rows;
        sa.bytes = src.a_buf; sa.w2 = nullptr; sa.kp = &src.kp; sa.off = valid ? src.a_start[pl.src] : 0; sa.dirty = false;
        sb.init(src.b_buf, src.kp, valid ? src.b_start[pl.src] : 0, valid ? (pl.swap ? pl.n : pl.m) : 0);
        if (valid && pl.swap) { rows = sb; cols = sa; } else { rows = sa; cols = sb; }
        int a5[RR];
#pragma unroll
        for (int r = 0; r < RR; r++) {
            int a = 5;
            const int q = q0 + r;
            if (valid && q >= P) { a = rows.at(q - P); if (a >= 5) { bad = 1; a = 4; } }
            a5[r] = a;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 5; b++) {
#pragma unroll
            for (int k = 0; k < RR / 2; k++) {
                const int x0 = a5[2 * k] >= 5 ? 25 : (pl.swap ? b * 5 + a5[2 * k] : a5[2 * k] * 5 + b);
                const int x1 = a5[2 * k + 1] >= 5 ? 25 : (pl.swap ? b * 5 + a5[2 * k + 1] : a5[2 * k + 1] * 5 + b);
                prof[b * SS_PLANE + lane * SS_LW + k] = (lds[x0] & 0xffff) | (lds[x1] << 16);
            }
        }
    }
    // column 0 (see the head of the file): real row: h' = D' = o, I'(i,1) = 2o; padding: h' = I' = o; the slot above row 1: h'(0,0) = 0
    // LOCAL: row 0 and every padding slot hold h = 0, rebased -e * (slot - P + 1); their I' starts at h' + o (a gap that never wins)
    auto hcol0 = [&](int q) { if constexpr (LOCAL) return q >= P ? O : -sp_e * (q - P + 1); else return (AFF && q != P - 1) ? O : 0; };
    int rt[RR], hold[RR];
#pragma unroll
    for (int r = 0; r < RR; r++) {
        hold[r] = hcol0(q0 + r);
        if constexpr (LOCAL) rt[r] = (q0 + r >= P) ? 2 * O : hcol0(q0 + r) + O;
        else rt[r] = (q0 + r >= P) ? 2 * O : O;
    }
    int diag0 = hcol0(q0 - 1);
    int dn_out = 0, h_out = 0;
    int up_dn = 2 * O, up_h = O; // level 0: the first lane keeps the row-0 constants as the `old` operand of its DPP moves
    SweepLocal<LOCAL> lo;
    if constexpr (LOCAL) {
        lo.zrow = sp_e * P; lo.bshift = O - sp_e; lo.end_t = lp;
        asm volatile("v_mov_b32 %0, %1" : "=v"(lo.vE) : "s"(sp_e));
    }
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
    auto load_col = [&](int j, int *w) { // MATRIX: this lane's entries of column j
        static_assert(!MAT || NW == 5, "a lane's entries are one 16-byte and one 4-byte load");
        const unsigned idx = (unsigned)(min(max(j, 1), m_c) - 1);
        const char *p = cbase + (unsigned long long)idx * cstride;
        const ss_int4 v = *reinterpret_cast<const ss_int4 *>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        w[4] = *reinterpret_cast<const int *>(p + 16);
    };
    auto col_raw = [&](int c) { return (c >= 1 && c <= m_eff) ? cols.raw(c - 1) : 0; };
    auto col_off = [&](int raw, int c) {
        int b = 0;
        if (c >= 1 && c <= m_eff) { b = cols.value(raw, c - 1); if (b >= 5) { bad = 1; b = 4; } }
        return b * (SS_PLANE * 4);
    };
    auto rb_at = [&](int c) { return (TAKES && c >= 1 && c <= m_eff) ? rb_load(&rb_in[c], piped) : make_int2(0, 0); };
    // ring_put(c0, ..): this lane's column c0 + lp goes into the rings (what was loaded a chunk earlier)
    auto ring_put = [&](int c0, int raw, int2 rq) {
        const int c = c0 + lp;
        if constexpr (!MAT) bring[c & (SS_RING - 1)] = col_off(raw, c);
        if (TAKES) hring[c & (SS_RING - 1)] = rq;
    };
    // prologue: columns 0 .. 31 into the rings, the loads of columns 32 .. 47 in flight
    int nraw = 0;
    int2 rqn = make_int2(0, 0);
    if (!MAT || TAKES) {
        if (TAKES) wait_cols(min(m_max, 47));
        ring_put(0, MAT ? 0 : col_raw(lp), rb_at(lp));
        ring_put(16, MAT ? 0 : col_raw(16 + lp), rb_at(16 + lp));
        if constexpr (!MAT) nraw = col_raw(32 + lp);
        rqn = rb_at(32 + lp);
        __syncthreads();
    }
    // the profile words of a step are read ONE STEP AHEAD (the base a lane needs at step t + 1 is the one the lane before it has at step t)
    int wq[SS_LW - 1];
    auto fetch = [&](int pbv, int *w) {
        const int2 *pw = reinterpret_cast<const int2 *>(prof_lane + pbv);
#pragma unroll
        for (int k = 0; k < (SS_LW - 1) / 2; k++) { const int2 v = pw[k]; w[2 * k] = v.x; w[2 * k + 1] = v.y; }
        w[SS_LW - 2] = *reinterpret_cast<const int *>(prof_lane + pbv + (SS_LW - 2) * 4);
    };
    int pb = 0, bnext = 0; // (ProfileSource)
    int ring[Src::D][NW]; // MATRIX: slot s holds the entries of the step at position s (mod D) of a chunk, loaded D steps ahead of their use
    if constexpr (MAT) {
#pragma unroll
        for (int s = 0; s < Src::D; s++) load_col(s - lp, ring[s]);
    } else {
        pb = bring[0];                 // base of step 0 (column 0 - lp <= 0: never used by a live cell)
        fetch(pb, wq);
        // the ring entries are read two steps / one step ahead of the DPP moves that use them
        bnext = bring[1];
    }
    int2 rq = TAKES ? hring[0] : make_int2(0, 0), rq1 = TAKES ? hring[1] : make_int2(0, 0); // what the first lane takes at steps 0 and 1

    auto step = [&](const int t, const int slot, auto chk) {
        constexpr bool CHECK = decltype(chk)::value; // false: every lane of the wave is inside its matrix
        if constexpr (LOCAL) {
            up_dn = dpp_shr1(TAKES ? rq.x : lo.zrow + vO, dn_out);
            up_h = dpp_shr1(TAKES ? rq.y : lo.zrow, h_out);
            lo.zrow -= lo.vE;
        } else {
            if (AFF) up_dn = dpp_shr1(TAKES ? rq.x : up_dn, dn_out);
            up_h = dpp_shr1(TAKES ? rq.y : up_h, h_out);
        }
        int pbn = 0, wn[SS_LW - 1];
        if constexpr (!MAT) {
            pbn = dpp_shr1(bnext, pb); // base of step t + 1
            bnext = bring[(t + 2) & (SS_RING - 1)];
        }
        if (TAKES) { rq = rq1; rq1 = hring[(t + 2) & (SS_RING - 1)]; }
        if constexpr (MAT) {
#pragma unroll
            for (int k = 0; k < NW; k++) wq[k] = ring[slot][k];
            load_col(t + Src::D - lp, ring[slot]); // this slot's next use is D steps away
        } else fetch(pbn, wn);
        asm volatile("" ::: "memory"); // the reads stay HERE, ahead of the arithmetic
        const int j = t - lp;
        if (!CHECK || (j >= 1 && j <= m_eff)) {
            int hd = diag0, dnu = AFF ? up_dn : up_h;
#pragma unroll
            for (int r = 0; r < RR; r++) {
                const int S = (r & 1) ? (wq[r >> 1] >> 16) : (int)(short)(wq[r >> 1] & 0xffff);
                const int M = hd + S;
                hd = hold[r];
                if constexpr (LOCAL) if (r == RR - 1) { // the last slot of a lane: row n in the last lane of the last level (elsewhere the result is not read)
                    const int cand = max(M, dnu);
                    lo.end_t = cand >= lo.bshift ? t : lo.end_t;
                    lo.bshift = max(cand, lo.bshift) - lo.vE;
                }
                if (AFF) {
                    const int hnew = max3i(M, rt[r], dnu);
                    const int ho = hnew + vO;
                    rt[r] = max(ho, rt[r]);
                    dnu = max(ho, dnu);
                    hold[r] = hnew;
                } else {
                    dnu = max3i(M, hold[r], dnu); // h'(i,j): the value the row below takes as its vertical candidate
                    hold[r] = dnu;
                }
            }
            diag0 = up_h;
            dn_out = dnu;
            h_out = hold[RR - 1];
            if (HANDS) { if (lp == G - 1) hand[t & 15] = make_int2(dn_out, h_out); }
        }
        if constexpr (!MAT) {
#pragma unroll
            for (int k = 0; k < SS_LW - 1; k++) wq[k] = wn[k];
            pb = pbn;
        }
    };
    auto chunk_head = [&](int t0) { // rings: columns t0 + 16 .. t0 + 31 from the loads of the chunk before; loads of t0 + 32 .. t0 + 47
        if (!MAT || TAKES) {
            if constexpr (MAT) hring[(t0 + 16 + lp) & (SS_RING - 1)] = rqn;
            else ring_put(t0 + 16, nraw, rqn);
            if (TAKES) wait_cols(min(m_max, t0 + 47));
            if constexpr (!MAT) nraw = col_raw(t0 + 32 + lp);
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
    // chunks of 16 steps; the steady ones (every lane of the wave inside its matrix) run without the per-lane test.  An edge chunk of
    // a source with a register ring is a loop over groups of D steps, so that the slot of a step stays a compile-time position
    const int Tend = ((m_max + G - 1) / 16 + 1) * 16;
    for (int t0 = 0; t0 < Tend; t0 += 16) {
        if (t0 > 0) chunk_head(t0);
        if (t0 >= 16 && t0 + 15 <= m_min) {
#pragma unroll
            for (int u = 0; u < 16; u++) step(t0 + u, u & (Src::D - 1), std::false_type{});
        } else if constexpr (Src::D == 1) {
#pragma unroll 1
            for (int u = 0; u < 16; u++) step(t0 + u, 0, std::true_type{});
        } else {
#pragma unroll 1
            for (int u0 = 0; u0 < 16; u0 += Src::D) {
#pragma unroll
                for (int s = 0; s < Src::D; s++) step(t0 + u0 + s, s, std::true_type{});
            }
        }
        hand_down(t0);
    }
    if (HANDS && piped) rb_publish(prog_out, 0x7fffffff, lane);
    if constexpr (LOCAL) {
        if (!HANDS && lp == G - 1 && valid) {
            outs.score()[pl.src] = (int64_t)lo.bshift + (int64_t)sp_e * ((int64_t)pl.n + pl.m + 1);
            int64_t *out_end = outs.end();
            if (out_end) out_end[pl.src] = lo.end_t - lp;
        }
    } else if (!HANDS && lp == G - 1 && valid) out_score[pl.src] = (int64_t)hold[RR - 1] + (int64_t)sp_e * ((int64_t)pl.n + pl.m);
    if (bad) atomicOr(err, 1);
}

// pairs of one row block (the shorter sequence <= 16 * RR bases): one wave per quad
template <bool AFF>
__global__ __launch_bounds__(64) void score_sweep_kernel(const ScorePlan *__restrict__ plans, const uint8_t *__restrict__ a_buf, const int64_t *__restrict__ a_start,
                                                         const uint8_t *__restrict__ b_buf, const int64_t *__restrict__ b_start, KParams kp, ScoreParams sp,
                                                         int64_t *__restrict__ out_score, int *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) int lds[SS_LDS];
    score_table_to_lds(lds, &sp);
    score_sweep_body<SS_RR, AFF>(lds, (int)blockIdx.x, plans, ProfileSource{a_buf, a_start, b_buf, b_start, kp}, sp.o, sp.e, out_score, err, nullptr, 0, false, false, false, nullptr, nullptr);
}

// The workgroup loop of the levels kernels (quads of S >= 2 row blocks).  The grid holds n_levels levels of W quads, level-major
// (block index = level * W + quad).
//   piped = 1: ONE launch for all levels (level0 = 0, n_levels = S); quad w of a level follows quad w of the level above through
//              prog[level * W + w]; nobody waits for a level that has not been taken (claim_items, gnx_common.hip.h): the claim words
//              sit behind the S * W progress words.
//   piped = 0: one launch per level in turn (n_levels = 1): nothing to wait for (GNX_NO_PIPE, and the fallback after a timeout).
// The arguments are ONE struct (Args: S, W, level0, piped, prog and what the body takes), and every level the workgroup runs reads
// them afresh from the kernel-argument segment (the pointer is made opaque per iteration): kept in scalar registers across the loop
// over stolen levels they do not fit beside the body's own.
//   to_lds(ka): what the kernel puts into LDS once (the score table, or nothing)
//   kparams(ka): the level's copy of the packed-reference pointers (or nothing), read before the barrier between two levels
//   body(ka, kp, quad, level, takes, hands, prog_in, prog_out): one level of one quad
template <class Args, class ToLds, class KP, class Body>
__device__ __forceinline__ void sweep_levels(ToLds to_lds, KP kparams, Body body) {
    typedef const __attribute__((address_space(4))) Args *ArgPtr;
    ArgPtr ka = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const int W = ka->W;
    const int lv_own = (int)blockIdx.x / W, w = (int)blockIdx.x - lv_own * W;
    int n_stolen = 0;
    if (ka->piped) { n_stolen = claim_items(ka->prog + (int64_t)ka->S * W, W, lv_own); if (n_stolen < 0) return; }
    to_lds(ka);
    for (int lv = lv_own - n_stolen; lv <= lv_own; lv++) {
        asm volatile("" : "+s"(ka));
        const int S = ka->S, Wk = ka->W, level = ka->level0 + lv;
        int *po = ka->prog + (int64_t)level * Wk + w;
        const int *pi = po - Wk;
        const auto kp = kparams(ka);
        if (lv != lv_own - n_stolen) __syncthreads(); // the LDS of the level before is no longer read
        body(ka, kp, w, level, level > 0, level < S - 1, pi, po);
    }
}
// kparams of the kernels whose source is the profile: all the sweep reads of KParams
struct LevelsKParams {
    template <class ArgPtr> __device__ __forceinline__ KParams operator()(ArgPtr ka) const {
        KParams kp;
        kp.b2 = ka->kp.b2; kp.bflag = ka->kp.bflag; kp.brank = ka->kp.brank; kp.bexc = ka->kp.bexc;
        return kp;
    }
};

struct ScoreLevelsArgs {
    const ScorePlan *plans; const uint8_t *a_buf; const int64_t *a_start; const uint8_t *b_buf; const int64_t *b_start;
    KParams kp; ScoreParams sp;
    int64_t *out_score; int *err; int2 *rowbuf;
    int S, W, level0, piped;
    int *prog;
};
template <bool AFF>
__global__ __launch_bounds__(64) void score_sweep_levels_kernel(ScoreLevelsArgs by_value) {
    __shared__ __attribute__((aligned(16))) int lds[SS_LDS];
    (void)by_value;
    sweep_levels<ScoreLevelsArgs>([&](auto ka) { score_table_to_lds(lds, &ka->sp); }, LevelsKParams(),
                                  [&](auto ka, const KParams &kp, int w, int level, bool takes, bool hands, const int *pi, int *po) {
        score_sweep_body<SS_RR, AFF>(lds, w, ka->plans, ProfileSource{ka->a_buf, ka->a_start, ka->b_buf, ka->b_start, kp}, ka->sp.o, ka->sp.e, ka->out_score, ka->err, ka->rowbuf,
                                     level, takes, hands, ka->piped != 0, pi, po);
    });
}

// ---- AffineGapLocal: score and target end ------------------------------------------------------------------
// The same sweep with LOCAL set: rows (lanes) are always the QUERY, columns the target whose ends are free (ScorePlan::swap only says
// which of the two buffers holds the rows).  Row 0 and the padding above it hold h = 0 on every column (profile entry -2e: a diagonal
// move of score 0; needs gapOpen <= 0 and gapExtend <= 0), the last row keeps the running maximum of max(M, I) over the columns and
// the column of its last >= update: the score of AffineGapLocal(target, query) and the target position behind its last aligned column.
__global__ __launch_bounds__(64) void score_local_kernel(const ScorePlan *__restrict__ plans, const uint8_t *__restrict__ a_buf, const int64_t *__restrict__ a_start,
                                                         const uint8_t *__restrict__ b_buf, const int64_t *__restrict__ b_start, KParams kp, ScoreParams sp,
                                                         int64_t *__restrict__ out_score, int64_t *__restrict__ out_end, int *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) int lds[SS_LDS];
    score_table_to_lds<true>(lds, &sp);
    struct Outs { int64_t *s, *e; __device__ __forceinline__ int64_t *score() const { return s; } __device__ __forceinline__ int64_t *end() const { return e; } };
    score_sweep_body<SS_RR, true, true>(lds, (int)blockIdx.x, plans, ProfileSource{a_buf, a_start, b_buf, b_start, kp}, sp.o, sp.e, nullptr, err, nullptr, 0, false, false, false, nullptr, nullptr, Outs{out_score, out_end});
}

struct ScoreLocalLevelsArgs {
    const ScorePlan *plans; const uint8_t *a_buf; const int64_t *a_start; const uint8_t *b_buf; const int64_t *b_start;
    KParams kp; ScoreParams sp;
    int64_t *out_score; int64_t *out_end; int *err; int2 *rowbuf;
    int S, W, level0, piped;
    int *prog;
};
template <class ArgPtr> struct LocalLevelsOuts {
    ArgPtr ka;
    __device__ __forceinline__ int64_t *score() const { return ka->out_score; }
    __device__ __forceinline__ int64_t *end() const { return ka->out_end; }
};
__global__ __launch_bounds__(64) void score_local_levels_kernel(ScoreLocalLevelsArgs by_value) {
    __shared__ __attribute__((aligned(16))) int lds[SS_LDS];
    (void)by_value;
    sweep_levels<ScoreLocalLevelsArgs>([&](auto ka) { score_table_to_lds<true>(lds, &ka->sp); }, LevelsKParams(),
                                       [&](auto ka, const KParams &kp, int w, int level, bool takes, bool hands, const int *pi, int *po) {
        score_sweep_body<SS_RR, true, true>(lds, w, ka->plans, ProfileSource{ka->a_buf, ka->a_start, ka->b_buf, ka->b_start, kp}, ka->sp.o, ka->sp.e, nullptr, ka->err, ka->rowbuf,
                                            level, takes, hands, ka->piped != 0, pi, po, LocalLevelsOuts<decltype(ka)>{ka});
    });
}

} // namespace
