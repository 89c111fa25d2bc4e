// span_origin.hip.h -- stage 2 of gnx_locate_span_*: the target START of AffineGapLocal's route, without a direction matrix
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.19.
#pragma once
#include "lat_fill.hip.h"    // wave_shr1
#include "score_sweep.hip.h" // ScorePlan

namespace {
// ------------------------------------------------------------------------------------------------------
// The local sweep (score_local_kernel, stage 1) has left the score S and the target end of every pair on the device.  The route lies
// inside target[lo : end] (the lemma), and the three-state recurrence of affineGap_highMem(freeEndGaps = true) over that
// window alone follows the reference's route, ties included.  This kernel runs it and carries, instead of a direction, the ORIGIN of
// every state: the window row at which the state's path left column 0.  start = lo + origin of the winner of (M, I) at (end, m).
//   lo          computed here, per pair, from S, end, m, smax+ = max(0, largest matrix entry), gapOpen and gapExtend:
//               dmax = floor((m smax+ + gapOpen - S) / -gapExtend) clamped at 0, lo = max(0, end - m - dmax); gapExtend == 0: lo = 0.
//               The number of steps of a pair is therefore known on the device only.
//   Geometry    one pair per wave at a time (the grid is a fixed number of waves that stride over the sub-batch's pairs); lane l owns
//               the SPAN_CPL = 3 query columns base + 3 l + 1 .. base + 3 l + 3 of a strip of 192 columns and walks down the window
//               rows, one anti-diagonal of lanes per step; the three keys and three origins of its LAST column and the target base
//               move to the next lane with `wave_shr:1` (lat_fill.hip.h).  No LDS.  (One column per lane, the first version, took
//               three strips and 3 x 63 ramp steps for a 150-base read: 7.7 ms for 100 000 pairs.)
//   Boundary    column 0: M = I = SENT, D = 0 with origin = its own row ("a state that leaves column 0 takes the row it leaves from");
//               row 0: M = D = SENT, I = gapOpen + j gapExtend, origin 0; the window's corner M = 0, I = gapOpen, D = 0, origin 0.
//               SENT = NEG4 = -2^30: finite keys stay above -2^29 under the sweep's static bound, one penalty added to SENT neither wins
//               nor wraps.
//   Ties        M >= I >= D at each of the three maxima, as compare + select on (key, origin) -- v_max3 would lose the origin.
//   Strips      a query of more than 192 bases takes ceil(m / 192) strips, one after the other in the same wave; lane 63 stores the six
//               values of its last column at every window row into the wave's hand-over rows (six arrays of `wcap` ints), the next
//               strip's lane 0 reads them back 64 rows at a time (one row per lane, then v_readlane per step) -- in place: a strip
//               stores row t - 63 at step t, after it has loaded rows t .. t + 63.  The last query column's D state (the free
//               trailing gap) feeds nothing that is read and takes the ordinary rule.
//   Self-check  max(M, I)(end, m) must equal stage 1's S; a difference sets err bit 64 (GNX_ETRACE on the host), as does a window
//               that does not fit the hand-over rows the host sized from its own bound on lo.
// Route 10 serves what the local sweep serves: queries up to 10 240 bases.
// ------------------------------------------------------------------------------------------------------
constexpr int SPAN_ERR = 64;               // bit of the sweep's error word
constexpr int SPAN_CPL = 3;                // query columns per lane
constexpr int SPAN_STRIP = 64 * SPAN_CPL;  // query columns per strip: a 150-base read is one strip and touches no hand-over row

struct SpanParams {
    int sc[25]; // scores[target * 5 + query]
    int o, e;   // gapOpen, gapExtend (both <= 0)
    int smaxp;  // max(0, largest matrix entry)
};
struct SpanArgs {
    const ScorePlan *plans; int n_plans;                  // the sweep's plans: n = query length, m = target length, src; n == 0: empty slot
    const uint8_t *t_buf; const int64_t *t_start;         // targets: plain bytes, or windows of the packed reference (kp.b2 != nullptr)
    const uint8_t *q_buf; const int64_t *q_start;         // queries: plain bytes
    KParams kp;
    SpanParams sp;
    const int64_t *score; const int64_t *end;             // stage 1's results
    int64_t *start;                                       // out
    int *err;
    int *hand; int wcap;                                  // per wave of the grid 6 * wcap ints (wcap == 0: no query is longer than a strip)
};

// (key, origin) of the first of a, b, c that is the maximum
__device__ __forceinline__ void span_pick(int a, int oa, int b, int ob, int c, int oc, int &best, int &org) {
    best = a; org = oa;
    if (b > best) { best = b; org = ob; }
    if (c > best) { best = c; org = oc; }
}
// SpanParams::sc[t * 5 + q] for a per-lane q without indexing the argument segment by a vector register
__device__ __forceinline__ int span_score(const SpanParams &sp, int t, int q) {
    int v = sp.sc[t * 5];
    v = q == 1 ? sp.sc[t * 5 + 1] : v;
    v = q == 2 ? sp.sc[t * 5 + 2] : v;
    v = q == 3 ? sp.sc[t * 5 + 3] : v;
    v = q >= 4 ? sp.sc[t * 5 + 4] : v;
    return v;
}

__global__ __launch_bounds__(64) void span_origin_kernel(SpanArgs a) {
    constexpr int C = SPAN_CPL;
    const int lane = threadIdx.x;
    const int o = a.sp.o, e = a.sp.e, oe = o + e;
    int *const hand = a.hand + (size_t)blockIdx.x * 6 * (size_t)a.wcap;
    for (int pi = (int)blockIdx.x; pi < a.n_plans; pi += (int)gridDim.x) {
        const ScorePlan pl = a.plans[pi];
        if (pl.n <= 0) continue;
        const int m = pl.n, n = pl.m;
        const int64_t S = a.score[pl.src];
        const int64_t end64 = a.end[pl.src];
        const int end = end64 < 0 ? 0 : (end64 > n ? n : (int)end64);
        int lo = 0;
        if (e < 0) {
            const int64_t num = (int64_t)m * a.sp.smaxp + o - S;
            const int64_t dmax = num > 0 ? num / -(int64_t)e : 0;
            const int64_t l = (int64_t)end - m - dmax;
            lo = l > 0 ? (int)l : 0;
        }
        const int W = end - lo; // window rows 1 .. W = target[lo .. end)
        const int strips = (m + SPAN_STRIP - 1) / SPAN_STRIP;
        if (strips > 1 && W >= a.wcap) { if (lane == 0) atomicOr(a.err, SPAN_ERR); continue; }
        BetaSrc T;
        T.init(a.t_buf, a.kp, a.t_start[pl.src], n);
        const uint8_t *q = a.q_buf + a.q_start[pl.src];
        int uM[C], uI[C], uD[C], ouM[C], ouI[C], ouD[C]; // the lane's columns at its last row; after the last strip: row W
        for (int s = 0; s < strips; s++) {
            const int base = s * SPAN_STRIP;
            const int nl = (min(SPAN_STRIP, m - base) + C - 1) / C; // lanes in use
            const bool more = s + 1 < strips;
            const int j0 = base + lane * C + 1;                     // the lane's first column
            int s0[C], s1[C], s2[C], s3[C], s4[C]; // the column's scores against target base 0 .. 4
#pragma unroll
            for (int c = 0; c < C; c++) {
                const int qb = j0 + c <= m ? (int)q[j0 + c - 1] : 0;
                s0[c] = span_score(a.sp, 0, qb); s1[c] = span_score(a.sp, 1, qb); s2[c] = span_score(a.sp, 2, qb); s3[c] = span_score(a.sp, 3, qb); s4[c] = span_score(a.sp, 4, qb);
                // row 0 of the lane's columns
                uM[c] = NEG4; uI[c] = o + (j0 + c) * e; uD[c] = NEG4; ouM[c] = 0; ouI[c] = 0; ouD[c] = 0;
            }
            // row 0 of the column to the lane's left (the diagonal of its first row)
            int pM = j0 == 1 ? 0 : NEG4, pI = o + (j0 - 1) * e, pD = j0 == 1 ? 0 : NEG4, opM = 0, opI = 0, opD = 0;
            int tbase = 0, tchunk = 0;
            int hM = NEG4, hI = NEG4, hD = 0, ohM = 0, ohI = 0, ohD = 0; // column `base` at rows t .. t + 63, one row per lane
            const int steps = W + nl - 1;
            for (int t = 1; t <= steps; t++) {
                const int k = (t - 1) & 63;
                if (k == 0) {
                    const int r = t + lane;
                    const bool in = r <= W;
                    tchunk = in ? min(T.at((int64_t)lo + r - 1), 4) : 0; // (a base >= 5 is stage 1's to report)
                    if (s == 0) ohD = r;
                    else if (in) {
                        hM = hand[r]; hI = hand[a.wcap + r]; hD = hand[2 * a.wcap + r];
                        ohM = hand[3 * a.wcap + r]; ohI = hand[4 * a.wcap + r]; ohD = hand[5 * a.wcap + r];
                    }
                }
                // the left column at this lane's row: the neighbour's last column at its last row; lane 0 takes column `base` at row t
                const int LM = wave_shr1(__builtin_amdgcn_readlane(hM, k), uM[C - 1]), LI = wave_shr1(__builtin_amdgcn_readlane(hI, k), uI[C - 1]),
                          LD = wave_shr1(__builtin_amdgcn_readlane(hD, k), uD[C - 1]);
                const int oLM = wave_shr1(__builtin_amdgcn_readlane(ohM, k), ouM[C - 1]), oLI = wave_shr1(__builtin_amdgcn_readlane(ohI, k), ouI[C - 1]),
                          oLD = wave_shr1(__builtin_amdgcn_readlane(ohD, k), ouD[C - 1]);
                tbase = wave_shr1(__builtin_amdgcn_readlane(tchunk, k), tbase);
                const int i = t - lane;
                if (i >= 1 && i <= W && lane < nl) {
                    int dM = pM, dI = pI, dD = pD, odM = opM, odI = opI, odD = opD; // the diagonal: the column to the left at the row above
                    int lM = LM, lI = LI, lD = LD, olM = oLM, olI = oLI, olD = oLD; // the column to the left at this row
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        int sv = s0[c];
                        sv = tbase == 1 ? s1[c] : sv; sv = tbase == 2 ? s2[c] : sv; sv = tbase == 3 ? s3[c] : sv; sv = tbase == 4 ? s4[c] : sv;
                        int nM, onM, nI, onI, nD, onD;
                        span_pick(dM, odM, dI, odI, dD, odD, nM, onM);
                        nM += sv;
                        span_pick(lM + oe, olM, lI + e, olI, lD + oe, olD, nI, onI);
                        span_pick(uM[c] + oe, ouM[c], uI[c] + oe, ouI[c], uD[c] + e, ouD[c], nD, onD);
                        dM = uM[c]; dI = uI[c]; dD = uD[c]; odM = ouM[c]; odI = ouI[c]; odD = ouD[c];
                        uM[c] = nM; uI[c] = nI; uD[c] = nD; ouM[c] = onM; ouI[c] = onI; ouD[c] = onD;
                        lM = nM; lI = nI; lD = nD; olM = onM; olI = onI; olD = onD;
                    }
                    pM = LM; pI = LI; pD = LD; opM = oLM; opI = oLI; opD = oLD;
                    if (more && lane == 63) {
                        hand[i] = lM; hand[a.wcap + i] = lI; hand[2 * a.wcap + i] = lD;
                        hand[3 * a.wcap + i] = olM; hand[4 * a.wcap + i] = olI; hand[5 * a.wcap + i] = olD;
                    }
                }
            }
            if (strips > 1) __syncthreads(); // the next strip (and the next pair's first strip) reads / overwrites what this one stored
        }
        const int cm = (m - 1) % SPAN_STRIP; // column m inside the last strip
        if (lane == cm / C) {
            int fM = uM[0], fI = uI[0], ofM = ouM[0], ofI = ouI[0];
#pragma unroll
            for (int c = 1; c < C; c++) if (cm % C == c) { fM = uM[c]; fI = uI[c]; ofM = ouM[c]; ofI = ouI[c]; }
            const bool takeM = fM >= fI;
            if ((int64_t)(takeM ? fM : fI) != S) atomicOr(a.err, SPAN_ERR);
            a.start[pl.src] = (int64_t)lo + (takeM ? ofM : ofI);
        }
    }
}

} // namespace
