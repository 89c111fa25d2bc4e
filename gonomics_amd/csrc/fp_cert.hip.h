// fp_cert.hip.h -- fast path: gapless reads leave by certificate before the sweep (scan + certify, live-list gather)
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.22.
#pragma once
#include "gnx_common.hip.h"
#include "fp_cert_decide.h"

namespace {
// ------------------------------------------------------------------------------------------------------
// A read that matches its window without an indel, with a mismatch deficit below two gap opens and no second copy in the window has a provably
// unique optimal alignment: leading gap, one diagonal, trailing gap (a few trailing bases possibly on the window's last columns).
// fp_cert_kernel proves that per pair -- one wave per pair -- and writes score, run count and staged runs exactly as fp_walk_kernel
// would have; every other pair gets live[p] = 1 and goes through sweep and walk as before.
//   1. the read's n - 15 16-mers (2 bits per base) go into an open-addressing table in LDS (512 slots, full key compare) with a
//      16 384-bit prefilter beside it; a 16-mer that holds an N is left out (two bits cannot say N): an N row is in no exact run;
//   2. the window is streamed 16 columns per lane and round (one 16-byte load, or one dword of the packed reference): a lane packs
//      its columns into a 32-bit code word, takes the word of the lane before it (__shfl_up) and looks up the 16 16-mers that START in
//      that earlier word's last 15 columns or at its own first one (v_alignbit): sixteen prefilter tests without a branch, then one
//      loop over the bits that are set.  Bytes that are not A C G T count as their two low bits: a false hit can only refuse a pair,
//      the decision below re-scores from the real bytes;
//   3. all hits must share one diagonal c (wave-wide min == max); a read that holds a 16-mer twice puts two hits on two diagonals;
//   4. the decision (fp_cert_decide.h, the pieces gnx_cert_decide is made of) runs across the wave: a lane takes ceil(n / 64) consecutive
//      rows -- the read's base from LDS, the window's bases on diagonal c, on its first and on its last columns from memory -- and the
//      lanes' sums are combined in int64 by wave sums and prefix scans (__shfl on the two halves): the deficit and the score by sums,
//      "no prefix of f above 0" by a scan of f, d* by a scan of g and a wave-wide (least prefix, first row), the edge rule's four
//      sums by masked sums once the deficit has fixed T1 and T2, the read's N rows (nu of the thresholds) by a sum.  The call's matrix
//      comes as a kernel argument (built once on the host).  A certified pair whose read holds an N adds one to *n_cert (one atomic);
//   5. a pair that fails the edge rule's corners and nothing else gets the corners graded by the real bytes on diagonals 0 and m - n
//      (gnx_certe_*: scans of the chunks' non-free counts, a ballot for the lane that holds the (j + 1)-th non-free row, E from a prefix
//      scan of the chunks' losses read by readlane); one it admits adds one to n_cert[1] instead.
// Windows of the packed reference that hold an exception (N, byte >= 5) are not certified; bytes >= 5 raise the sweep's error flag.
// ------------------------------------------------------------------------------------------------------
constexpr int CERT_K = 16;
constexpr int CERT_SLOTS = 512;  // table slots (at most 145 keys); the prefilter has 32 bits per slot word
constexpr int CERT_NMAX = 160;   // one row block
constexpr int CERT_CHUNK = (CERT_NMAX + 63) / 64; // rows per lane, at most

// wave operations of the decision (tests/cpp/cert_wave_test.cpp restates them on the host, in this order)
__device__ __forceinline__ int64_t cert_wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int64_t cert_wave_scan(int64_t v, int lane) { // inclusive prefix sums
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int64_t t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}

__device__ __forceinline__ int cert_wave_scan32(int v, int lane) { // inclusive prefix sums of small counts
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ int64_t cert_read_lane64(int64_t v, int src) { // lane src's value, src uniform
    const int s = __builtin_amdgcn_readfirstlane(src);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(uint64_t)v, s), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((uint64_t)v >> 32), s);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ unsigned cert_hash(unsigned code) { return code * 0x9E3779B1u; } // slot = top 9 bits, filter bit = top 14 bits
// 2-bit codes of four dna.Base bytes -> 8 bits (byte k at bits 2k)
__device__ __forceinline__ unsigned cert_pack4(unsigned w) {
    unsigned x = w & 0x03030303u;
    x = (x | (x >> 6)) & 0x000F000Fu;
    return (x | (x >> 12)) & 0xFFu;
}

template <bool PK>
__global__ __launch_bounds__(64) void fp_cert_kernel(const PairPlan *__restrict__ plans, int n_pairs,
                                                     const uint8_t *__restrict__ a_buf, const int64_t *__restrict__ a_start,
                                                     const uint8_t *__restrict__ b_buf, const int64_t *__restrict__ b_start,
                                                     KParams kp, TbParams tp, GnxCertMatrix mx, gnx_cigar *__restrict__ stage, int cap,
                                                     int64_t *__restrict__ score_out, int64_t *__restrict__ nops,
                                                     int64_t *__restrict__ live, int64_t *__restrict__ n_cert, int *__restrict__ err) {
    __shared__ unsigned keys[CERT_SLOTS];
    __shared__ int qv[CERT_SLOTS];
    __shared__ unsigned filt[CERT_SLOTS];
    __shared__ uint8_t sa[CERT_NMAX];
    __shared__ int64_t sw[40]; // w(x, y) at 8 x + y, x = 4: the N row (the host built mx with mx.ok set, or did not launch)
    const int p = (int)blockIdx.x;
    if (p >= n_pairs) return;
    const int lane = threadIdx.x;
    const PairPlan pl = plans[p];
    const int n = pl.n, m = pl.m;
    bool bad = false;
    bool out = n < CERT_K || n > CERT_NMAX || m < n + 2 || kp.o4 >= 0 || tp.ci < n || tp.cj < m; // (wave-uniform)
    BetaSrcT<PK ? 1 : 0> bp;
    const int64_t boff = b_start[pl.src];
    bp.init(b_buf, kp, boff, m);
    if (PK && bp.dirty) out = true;
    if (out) { if (lane == 0) live[p] = 1; return; }
    const uint8_t *ap = a_buf + a_start[pl.src];

    // ---- 1. the read and its 16-mers ----
    for (int x = lane; x < CERT_SLOTS; x += 64) { qv[x] = -1; filt[x] = 0; }
    bool read_ok = true;
    for (int i = lane; i < n; i += 64) { const uint8_t v = ap[i]; sa[i] = v; if (v >= 5) read_ok = false; }
    if (__any(!read_ok)) { if (lane == 0) live[p] = 1; return; } // (a byte >= 5: the sweep flags it)
    if (lane < 40) sw[lane] = gnx_cert_table8_entry(&mx, lane);
    __syncthreads(); // (sa and the empty table, before the 16-mers are read and inserted)
    for (int q = lane; q + CERT_K <= n; q += 64) {
        unsigned code = 0, has_n = 0;
#pragma unroll
        for (int t = 0; t < CERT_K; t++) { const unsigned v = sa[q + t]; has_n |= v; code |= (v & 3u) << (2 * t); }
        if (has_n & 4u) continue; // (bytes are 0 .. 4 here)
        const unsigned h = cert_hash(code);
        unsigned slot = h >> 23;
        while (atomicCAS(&qv[slot], -1, q) != -1) slot = (slot + 1) & (CERT_SLOTS - 1); // (a key the read holds twice takes two slots)
        keys[slot] = code;
        atomicOr(&filt[h >> 23], 1u << ((h >> 18) & 31u));
    }
    __syncthreads();

    // ---- 2 and 3. the window, 16 columns per lane and round; all hits on one diagonal, aligned to the 16-byte / dword grid of its buffer ----
    const int sh = PK ? (int)(boff & 15) : (int)((uintptr_t)(b_buf + boff) & 15); // columns of the first group that lie before the window
    const int n_groups = (sh + m + 15) >> 4;
    const uint8_t *bw = b_buf + boff - sh;              // bytes: the first group's address (16-byte aligned)
    const unsigned *w2 = PK ? kp.b2 + (boff >> 4) : nullptr; // packed: the first group's dword
    auto load_group = [&](int g, bool &badv) -> unsigned {
        if (g >= n_groups) return 0u;
        if (PK) return w2[g];
        const int c0 = 16 * g - sh; // the group's first column (0-based in the window)
        if (c0 >= 0 && c0 + 16 <= m) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bw + 16 * (int64_t)g);
            const unsigned any = v.x | v.y | v.z | v.w | (v.x + 0x03030303u) | (v.y + 0x03030303u) | (v.z + 0x03030303u) | (v.w + 0x03030303u);
            if (any & 0xF8F8F8F8u) badv = true; // a byte >= 5 (>= 8 has a high bit set; 5 .. 7 get one by the add; a carry needs one already)
            return cert_pack4(v.x) | (cert_pack4(v.y) << 8) | (cert_pack4(v.z) << 16) | (cert_pack4(v.w) << 24);
        }
        unsigned cw = 0;
        for (int t = 0; t < 16; t++) {
            const int col = c0 + t;
            if (col >= 0 && col < m) { const unsigned v = bw[16 * (int64_t)g + t]; if (v >= 5) badv = true; cw |= (v & 3u) << (2 * t); }
        }
        return cw;
    };
    int dmin = 0x7fffffff, dmax = -0x7fffffff - 1;
    unsigned carry = 0;
    unsigned nxt = load_group(lane, bad);
    for (int g0 = 0; g0 < n_groups; g0 += 64) {
        const unsigned cw = nxt;
        nxt = load_group(g0 + 64 + lane, bad); // the next round's load is in flight while this one is looked up
        unsigned prev = __shfl_up(cw, 1, 64);
        if (lane == 0) prev = carry;
        carry = __shfl(cw, 63, 64);
        const int s0 = 16 * (g0 + lane) - sh - 16; // window column (0-based) of the earlier word's first base
        unsigned hits = 0; // bit t - 1: the prefilter has the 16-mer that starts t bases into `prev` -- sixteen tests without a branch
#pragma unroll
        for (int t = 1; t <= 16; t++) {
            const unsigned h = cert_hash(t < 16 ? __builtin_amdgcn_alignbit(cw, prev, 2 * t) : cw);
            hits |= ((filt[h >> 23] >> ((h >> 18) & 31u)) & 1u) << (t - 1);
        }
        while (hits) { // (one branch per round; about one lookup in a hundred gets here, and the read's own locus)
            const int t = __ffs(hits);
            hits &= hits - 1;
            const unsigned code = (unsigned)((((unsigned long long)cw << 32) | prev) >> (2 * t));
            const unsigned h = cert_hash(code);
            const int s = s0 + t;
            if (s >= 0 && s + CERT_K <= m) {
                unsigned slot = h >> 23;
                int q;
                while ((q = qv[slot]) != -1 && dmin >= dmax) {
                    if (keys[slot] == code) { dmin = min(dmin, s - q); dmax = max(dmax, s - q); }
                    slot = (slot + 1) & (CERT_SLOTS - 1);
                }
            }
        }
        if (__any(dmin < dmax)) break; // two diagonals: no certificate (the rest of the window's bytes are the sweep's to check)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { dmin = min(dmin, __shfl_xor(dmin, d, 64)); dmax = max(dmax, __shfl_xor(dmax, d, 64)); }
    if (bad) atomicOr(err, 1);
    const int c = dmin;
    if (dmin != dmax || c <= 0 || c >= m - n) { if (lane == 0) live[p] = 1; return; } // (no hit at all: dmin > dmax)

    // ---- 4. the decision across the wave: the real bases under a lane's rows on diagonal c, on the window's first and last columns ----
    const int chunk = (n + 63) >> 6, i0 = lane * chunk;
    GnxCertLane ln;
    gnx_cert_lane_init(&ln);
    int64_t loss[CERT_CHUNK];
#pragma unroll
    for (int k = 0; k < CERT_CHUNK; k++) {
        const int i = i0 + k;
        loss[k] = 0;
        if (k < chunk && i < n) loss[k] = gnx_certn_lane_row<8>(&ln, sw, mx.R[4], 1, i, sa[i], (unsigned)bp.at(c + i), (unsigned)bp.at(i), (unsigned)bp.at(m - n + i));
    }
    if (__any(!ln.ok)) { if (lane == 0) live[p] = 1; return; } // a byte >= 5 under the read
    int nu = 0; // the read's N rows: a wave sum of the chunks' counts, by ballots (scalar)
#pragma unroll
    for (int k = 0; k < CERT_CHUNK; k++) nu += __popcll(__ballot(ln.nn > k));
    const int64_t D = cert_wave_sum(ln.loss), mid_sum = cert_wave_sum(ln.mid);
    const int64_t Fi = cert_wave_scan(ln.f, lane), Gi = cert_wave_scan(ln.g, lane);
    const int f_pos = __any(ln.rows > 0 && Fi - ln.f + ln.f_top > 0); // some F_alpha > 0
    int64_t g_low = ln.rows > 0 ? Gi - ln.g + ln.g_low : INT64_MAX;
    int g_row = ln.rows > 0 ? ln.g_row : n;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) gnx_cert_low_min(&g_low, &g_row, __shfl_xor(g_low, d, 64), __shfl_xor(g_row, d, 64));
    const GnxCertBounds t = gnx_certn_bounds(mx.lambda, mx.o, n, CERT_K, D, nu); // (uniform from here on)
    int64_t h1 = 0, h2 = 0, t1 = 0, t2 = 0;
    if (t.edge) { // the loss of the first / last T1 and T2 rows
#pragma unroll
        for (int k = 0; k < CERT_CHUNK; k++) {
            const int i = i0 + k;
            if (i < t.T1) h1 += loss[k];
            if (i < t.T2) h2 += loss[k];
            if (i >= n - t.T1) t1 += loss[k];
            if (i >= n - t.T2) t2 += loss[k];
        }
        h1 = cert_wave_sum(h1); h2 = cert_wave_sum(h2); t1 = cert_wave_sum(t1); t2 = cert_wave_sum(t2);
    }
    int64_t best, ds, sc;
    gnx_cert_tail(__shfl(Gi, 63, 64), g_low, g_row, n, &best, &ds);
    bool by_edge = false; // admitted by the graded corners only
    if (!gnx_cert_finish(&t, mx.o, mx.e, n, m, f_pos, mid_sum, h1, h2, t1, t2, best, ds, &ds, &sc)) {
        // ---- 5. refused for the corners and for nothing else: the edge rule graded by the bytes on diagonals 0 and m - n (uniform) ----
        if (!(t.ok && !f_pos && t.edge && ds < n && (h1 + t2 >= -mx.o || h2 + t1 >= -mx.o))) { if (lane == 0) live[p] = 1; return; }
        GnxCertEdgeLane el;
        gnx_certe_lane_init(&el, i0);
#pragma unroll
        for (int k = 0; k < CERT_CHUNK; k++) {
            const int i = i0 + k;
            if (k < chunk && i < n) gnx_certe_lane_row(&el, sa[i], (unsigned)bp.at(i), (unsigned)bp.at(m - n + i));
        }
        const int inc0 = cert_wave_scan32(el.c0, lane), incm = cert_wave_scan32(el.cm, lane);
        const int before0 = inc0 - el.c0, afterm = __builtin_amdgcn_readlane(incm, 63) - incm;
        // P[k] = the loss of the first k rows: the lane of row k holds it (k0 before its first row)
        const int64_t k0 = cert_wave_scan(ln.loss, lane) - ln.loss;
        auto prefix = [&](int k) -> int64_t {
            if (k >= n) return D;
            const int L = k / chunk, r = k - L * chunk;
            int64_t v = k0; // (sums, not a choice of three values: nothing here may turn into a table in private memory)
#pragma unroll
            for (int x = 0; x + 1 < CERT_CHUNK; x++) v += r > x ? loss[x] : 0;
            return cert_read_lane64(v, L);
        };
        const int J30 = (int)gnx_certe_grades(mx.lambda, mx.o, D);
        bool pass = true;
        for (int j = 0; j <= J30 && pass; j++) {
            const int hr = gnx_certe_head_row(&el, before0, j), tr = gnx_certe_tail_row(&el, afterm, j);
            const unsigned long long bh = __ballot(hr >= 0), bt = __ballot(tr >= 0); // (one lane at most holds the row)
            const int A0 = bh ? __builtin_amdgcn_readlane(hr, __builtin_amdgcn_readfirstlane(__ffsll(bh) - 1)) : n;
            const int Am = bt ? n - 1 - __builtin_amdgcn_readlane(tr, __builtin_amdgcn_readfirstlane(__ffsll(bt) - 1)) : n;
            int64_t pq[4], ha, ta, hb, tb;
            gnx_certe_corners(CERT_K, nu, j, A0, Am, pq);
            gnx_certe_span(n, pq[0], pq[1], &ha, &ta);
            gnx_certe_span(n, pq[2], pq[3], &hb, &tb);
            pass = gnx_certe_grade(mx.lambda, mx.o, j, prefix((int)ha) + D - prefix((int)ta), prefix((int)hb) + D - prefix((int)tb)) != 0;
        }
        if (!pass) { if (lane == 0) live[p] = 1; return; }
        sc = mid_sum + best + 2 * mx.o + mx.e * ((int64_t)n + m);
        by_edge = true;
    }
    if (lane == 0) {
        // the runs in traceback order, as fp_walk_kernel stages them: [d* M] [m - n - c I] [n - d* M] [c I]
        gnx_cigar *stg = stage + (int64_t)p * cap;
        int cnt = 0;
        auto put = [&](int op, int64_t run) { gnx_cigar g; g.run_length = run; g.op = (uint8_t)op; for (int z = 0; z < 7; z++) g._pad[z] = 0; stg[cnt++] = g; };
        if (ds > 0) put(0, ds);
        put(1, (int64_t)m - n - c);
        put(0, (int64_t)n - ds);
        put(1, c);
        nops[p] = cnt;
        score_out[p] = sc;
        live[p] = 0;
        if (by_edge) atomicAdd(reinterpret_cast<unsigned long long *>(n_cert + 1), 1ull);
        else if (nu > 0) atomicAdd(reinterpret_cast<unsigned long long *>(n_cert), 1ull);
    }
}

// the live pairs in ascending order: list and gathered plans (off = exclusive scan of live[])
__global__ __launch_bounds__(256) void fp_cert_gather_kernel(int n_pairs, const int64_t *__restrict__ live, const int64_t *__restrict__ off,
                                                             const PairPlan *__restrict__ plans, int *__restrict__ list, PairPlan *__restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs || !live[p]) return;
    const int64_t k = off[p];
    list[k] = p;
    out[k] = plans[p];
}

} // namespace
