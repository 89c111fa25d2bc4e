// aln_md.hip.h -- gnx_md_*: the MD string of a finished alignment (contract: gnx_align.h)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).
//
// MD is the other standard encoding of the walk aln_summary_kernel makes: the one that carries the reference (alpha) LETTERS under
// every substitution and deletion.  The resident reference exists on the device only, packed, so the string is written here.
//
// Geometry: aln_summary_kernel's -- one wave per pair, four pairs per workgroup, the CIGAR in blocks of 64 runs loaded a block ahead,
// BetaSrcT sources with PK naming the packed side at compile time, no LDS, no scratch, no atomics.
//
// Events.  An EVENT is an inside column (AffineGapLocal's free end gaps are outside) that is an X column or a D column.  Its token is
//   X                             dec(i - q - 1) letter
//   D, column before no inside D  dec(i - q - 1) '^' letter
//   D behind an inside D column   letter
// with i its alpha position and q the alpha position of the event before it (alpha_start - 1 at first): I columns consume no alpha, so
// "equal columns since the last event" is a difference of alpha positions.  Whether the column before a D run is an inside D column is
// the summary's seam rule, a function of position alone: the op of the nearest run of non-zero length before it (adjacent D runs lie
// in the same maximal D run, so they are inside or outside together).  The string ends with dec(alpha_end - q - 1).
// So a token depends on (i, q, type, predecessor) and on nothing else: byte offsets are an exclusive SUM scan of token lengths and q is
// a MAX scan of event positions, over lanes, 64-column steps, runs and 64-run blocks -- the pair of scans the extended-CIGAR WRITE
// pass carries (slot and last start).  Positions are carried plus one (0: no event yet in this run).
//
// Per block of runs: a first walk gives every run its bytes WITHOUT the decimal of its first event, the position of that event and of
// its last one; the max scan gives each run the q of its first event and with it the missing digits; the sum scan gives its first
// byte.  aln_md_kernel<false> stops there (the pair's byte count; scan_kernel's family turns the counts into offsets),
// aln_md_kernel<true> walks again and stores.  The free end gaps are needed BEFORE the walk (the summary reads them after it), and
// with them the pair's column total: one pass over the run lengths, local mode only.
//
// Two forms of walking a run, as in the summary; the bytes cannot depend on which ran:
//   lane per run      each lane walks its own M run column by column and writes its own D run letter by letter.
//   lane per column   a run of at least `cut` columns is taken by the whole wave, 64 columns per step: substitutions as one ballot, the
//                     event before a lane's as the highest bit below it, byte offsets as a wave scan of the step's token lengths (steps
//                     without a substitution skip it); a D run has no decision to make -- one header, then 64 letters per step.
// The cut is 64 columns.  GNX_MD_FORM=0 sends every run to the lane-per-column form, =1 every one to the lane-per-run form (tests).
// Numbers are below 2^30: at most 10 digits.
#pragma once
#include "aln_summary.hip.h"

namespace {

struct MdArgs {
    SumArgs s;            // sequences, CIGARs, cut, local, n_pairs; nx = the byte counts (WRITE = false), xoff = each pair's first byte (WRITE = true)
    char *md;             // WRITE = true
};

__device__ __forceinline__ unsigned md_digits(unsigned v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ char md_letter(int x) { return (char)((0x4E54474341ull >> (8 * min(x, 4))) & 0xffull); } // "ACGTN" (a byte >= 5 fails the call before a letter is stored)
// dec(v) into out[at ..), nd = md_digits(v); returns the byte behind it
__device__ __forceinline__ unsigned md_put_dec(char *out, unsigned at, unsigned v, unsigned nd) {
    for (unsigned k = nd; k-- > 0;) { out[at + k] = (char)('0' + v % 10u); v /= 10u; }
    return at + nd;
}

// what the first walk of one run yields: its bytes without the decimal of its first event, the alpha position of that event plus one
// (0: the run has no event that prints a decimal first), the alpha position of its last event plus one (0: no event)
struct MdRun { unsigned cnt, first1, last1; };

// lane per run: this lane's M run of `len` columns from (i0, j0).  WRITE: q1 = the event before the run plus one, `at` = the run's first byte
template <bool WRITE, class SrcA, class SrcB>
__device__ __forceinline__ MdRun md_walk_run(const SrcA &A, const SrcB &B, int i0, int j0, int len, unsigned q1, char *out, unsigned at) {
    MdRun r = {0, 0, 0};
    int x = A.at(i0), y = B.at(j0); // (the bases of a column are loaded one column ahead)
    for (int k = 0; k < len; k++) {
        int nx = 0, ny = 0;
        if (k + 1 < len) { nx = A.at(i0 + k + 1); ny = B.at(j0 + k + 1); }
        if (x != y) {
            const unsigned i = (unsigned)(i0 + k);
            if (WRITE) {
                at = md_put_dec(out, at, i - q1, md_digits(i - q1));
                out[at++] = md_letter(x);
                q1 = i + 1;
            } else {
                if (r.last1 == 0) { r.first1 = i + 1; r.cnt = 1; }
                else r.cnt += md_digits(i - r.last1) + 1;
                r.last1 = i + 1;
            }
        }
        x = nx; y = ny;
    }
    return r;
}

// lane per column: the same run, every argument wave-uniform.  WRITE = false: cnt comes back PER LANE (the caller sums it over the
// wave), first1 / last1 uniform.
template <bool WRITE, class SrcA, class SrcB>
__device__ __forceinline__ MdRun md_walk_wave(const SrcA &A, const SrcB &B, int i0, int j0, int len, int lane, unsigned q1, char *out, unsigned at) {
    MdRun r = {0, 0, 0};
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned q = WRITE ? q1 : 0u; // the last event so far, plus one (WRITE = false: 0 = none in this run yet)
    bool valid = lane < len;
    int x = 0, y = 0;
    if (valid) { x = A.at(i0 + lane); y = B.at(j0 + lane); } // (the bases of a step are loaded one step ahead)
    for (int s = 0; s < len; s += 64) {
        const int k = s + lane;
        const bool nvalid = k + 64 < len;
        int nx = 0, ny = 0;
        if (nvalid) { nx = A.at(i0 + k + 64); ny = B.at(j0 + k + 64); }
        const unsigned long long xm = __ballot(valid && x != y);
        if (xm) { // (wave-uniform: most steps hold no substitution)
            const bool mine = (xm >> lane) & 1ull;
            const unsigned long long pm = xm & below;
            const unsigned i = (unsigned)(i0 + k);
            const unsigned qb = pm ? (unsigned)(i0 + s) + (64u - (unsigned)__clzll((long long)pm)) : q; // the event before this lane's, plus one
            if (WRITE) {
                const unsigned nd = md_digits(i - qb);
                unsigned total;
                const unsigned mine_at = at + sum_wave_scan(mine ? nd + 1u : 0u, lane, total);
                if (mine) out[md_put_dec(out, mine_at, i - qb, nd)] = md_letter(x);
                at += total;
            } else {
                if (mine) r.cnt += (qb == 0u) ? 1u : md_digits(i - qb) + 1u;
                if (q == 0u) r.first1 = (unsigned)(i0 + s) + (unsigned)__ffsll((long long)xm);
            }
            q = (unsigned)(i0 + s) + (64u - (unsigned)__clzll((long long)xm));
        }
        x = nx; y = ny; valid = nvalid;
    }
    r.last1 = q;
    return r;
}

// PK: which side is a window of the packed reference (aln_summary_kernel's rule: decided at run time both forms ran out of scalar registers)
template <bool WRITE, int PK>
__global__ __launch_bounds__(256) void aln_md_kernel(MdArgs m) {
    const SumArgs &a = m.s;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.n_pairs; p += (int64_t)gridDim.x * 4) {
        const int n = (int)a.a_len[p], mlen = (int)a.b_len[p];
        BetaSrcT<PK == 1 ? 1 : 0> A;
        BetaSrcT<PK == 2 ? 1 : 0> B;
        A.init(a.a_buf, a.kp, a.a_start[p], n);
        B.init(a.b_buf, a.kp, a.b_start[p], mlen);
        const int64_t r0 = a.ops_off[p], nr = a.ops_off[p + 1] - r0;
        char *out = WRITE ? m.md + a.xoff[p] : nullptr;
        // the inside columns: [lead, cend) -- everything unless the mode has free end gaps
        unsigned lead = 0, cend = 0xffffffffu;
        if (a.local) {
            unsigned cols = 0;
            for (int64_t rb = 0; rb < nr; rb += 64) cols += sum_wave_sum(rb + lane < nr ? (unsigned)a.ops[r0 + rb + lane].run_length : 0u);
            lead = sum_free_end(a.ops + r0, nr, lane, false);
            cend = cols - sum_free_end(a.ops + r0, nr, lane, true); // (one D run: lead = cols and cend = 0, nothing inside)
        }
        // carried from block to block, wave-uniform
        unsigned ci = 0, cj = 0, cc = 0;    // alpha bases, beta bases, columns so far
        int prev_op = -1;                   // op of the last run of non-zero length (-1: none yet)
        unsigned n_bytes = 0, last1 = lead; // bytes so far; the alpha position of the last event plus one (alpha_start at first)
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
            // the op of the column before this run's first column (the seam rule)
            const unsigned long long nzb = nz & below;
            int pop = __shfl(op, nzb ? 63 - __clzll((long long)nzb) : 0, 64);
            if (!nzb) pop = prev_op;
            const bool mrun = len > 0 && op == GNX_COL_M, drun = len > 0 && op == GNX_COL_D && c0 >= lead && c0 < cend;
            const bool head = drun && pop != GNX_COL_D; // this D run opens a ^ group
            const bool coop_m = mrun && len >= a.cut, coop_d = drun && len >= a.cut;
            // walk 1: every run's bytes (the decimal of its first event apart), its first and its last event
            MdRun r = {0, 0, 0};
            if (drun) { r.cnt = (unsigned)len + (head ? 1u : 0u); r.first1 = head ? (unsigned)i0 + 1u : 0u; r.last1 = (unsigned)(i0 + len); }
            if (mrun && !coop_m) r = md_walk_run<false>(A, B, i0, j0, len, 0u, nullptr, 0u);
            for (unsigned long long cm = __ballot(coop_m); cm; cm &= cm - 1) {
                const int o = __ffsll((long long)cm) - 1;
                const MdRun u = md_walk_wave<false>(A, B, __shfl(i0, o, 64), __shfl(j0, o, 64), __shfl(len, o, 64), lane, 0u, nullptr, 0u);
                const unsigned cnt = sum_wave_sum(u.cnt);
                if (lane == o) { r.cnt = cnt; r.first1 = u.first1; r.last1 = u.last1; }
            }
            unsigned tlast, tcnt;
            const unsigned q1 = sum_wave_maxscan(r.last1, lane, last1, tlast); // the event before this run's first, plus one
            if (r.first1) r.cnt += md_digits(r.first1 - 1u - q1);
            const unsigned at = n_bytes + sum_wave_scan(r.cnt, lane, tcnt);
            if (WRITE) { // walk 2: the bytes
                if (drun && !coop_d) {
                    unsigned w = at;
                    if (head) { w = md_put_dec(out, w, (unsigned)i0 - q1, md_digits((unsigned)i0 - q1)); out[w++] = '^'; }
                    for (int k = 0; k < len; k++) out[w + k] = md_letter(A.at(i0 + k));
                }
                if (mrun && !coop_m) (void)md_walk_run<true>(A, B, i0, j0, len, q1, out, at);
                for (unsigned long long cm = __ballot(coop_m); cm; cm &= cm - 1) {
                    const int o = __ffsll((long long)cm) - 1;
                    (void)md_walk_wave<true>(A, B, __shfl(i0, o, 64), __shfl(j0, o, 64), __shfl(len, o, 64), lane, __shfl(q1, o, 64), out, __shfl(at, o, 64));
                }
                for (unsigned long long cd = __ballot(coop_d); cd; cd &= cd - 1) { // a long D run: one header, then a lane per letter
                    const int o = __ffsll((long long)cd) - 1;
                    const int ui0 = __shfl(i0, o, 64), ulen = __shfl(len, o, 64);
                    const unsigned uq1 = __shfl(q1, o, 64);
                    unsigned w = __shfl(at, o, 64);
                    if (__shfl((int)head, o, 64)) {
                        const unsigned nd = md_digits((unsigned)ui0 - uq1);
                        if (lane == 0) out[md_put_dec(out, w, (unsigned)ui0 - uq1, nd)] = '^';
                        w += nd + 1u;
                    }
                    for (int k = lane; k < ulen; k += 64) out[w + k] = md_letter(A.at(ui0 + k));
                }
            }
            n_bytes += tcnt; last1 = tlast;
            ci += ti; cj += tj; cc += tc;
            if (nz) prev_op = __shfl(op, 63 - __clzll((long long)nz), 64);
        }
        // the closing decimal: the equal columns behind the last event, up to alpha_end
        const unsigned a_end = !a.local ? ci : (cc > 0 && lead == cc) ? lead : ci - (cc - cend); // (one free D run as a whole: alpha_start = alpha_end)
        const unsigned tail = a_end - last1, nd = md_digits(tail);
        if (lane == 0) {
            if (WRITE) (void)md_put_dec(out, n_bytes, tail, nd);
            else a.nx[p] = (int64_t)n_bytes + nd;
        }
    }
}

} // namespace
