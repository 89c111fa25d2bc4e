// fp_cert_decide.h -- the gapless-read certificate's decision arithmetic, plain C++: no HIP header needed.
// The pieces -- a row's terms, a lane's chunk of rows, the thresholds, the tail rule, the finishing arithmetic -- are shared by
// fp_cert_kernel (fp_cert.hip.h: 64 lanes with a chunk of rows each, combined by wave sums and scans) and by gnx_cert_decide, their serial
// composition, which the host-only debug entry gnx_debug_gapless_certificate runs (the CPU tests; tests/cpp/cert_wave_test.cpp
// evaluates the pieces the kernel's way on the host and requires gnx_cert_decide's results).  Exact integer arithmetic in int64.
// The gnx_certn_* pieces admit reads that hold N: an N row is never exact and never imperfect, it loses R_N - w(N, y) >= 0 on a cell
// and R_N >= 0 when skipped, and the nu N rows of the read enter the thresholds beside J.  There is one arithmetic: the gnx_cert_*
// pieces of the N-free rule are the gnx_certn_* ones with N refused (allow_n = 0, nu = 0), signatures and results as before.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNX_CERT_HD __host__ __device__
#else
#define GNX_CERT_HD
#endif
#define GNX_CERTE_HD GNX_CERT_HD __attribute__((always_inline)) // the graded edge rule's pieces: called in a loop of the kernel with their arguments in registers

// Per call, from gnx_params: w(x, y) = s(x, y) - 2e (the rebasing of section 4), R_x = w(x, x), lambda = the least loss of a read row
// that is mismatched or skipped and is not N; R[4] = R_N = max(0, max_y w(N, y)), so that an N row loses >= 0 wherever it lies.
// ok = 0: the matrix (or gapOpen >= 0) admits no certificate.
struct GnxCertMatrix {
    int64_t w[25];
    int64_t R[5];
    int64_t lambda;
    int64_t o, e;
    int32_t ok;
};

GNX_CERT_HD inline void gnx_cert_matrix_init(GnxCertMatrix *mx, const int64_t *scores, int64_t gap_open, int64_t gap_extend) {
    mx->o = gap_open; mx->e = gap_extend;
    for (int x = 0; x < 25; x++) mx->w[x] = scores[x] - 2 * gap_extend;
    int ok = gap_open < 0 ? 1 : 0;
    int64_t lam = INT64_MAX;
    for (int x = 0; x < 4; x++) {
        const int64_t Rx = mx->w[x * 5 + x];
        int64_t worst = INT64_MIN;
        for (int y = 0; y < 5; y++) if (y != x && mx->w[x * 5 + y] > worst) worst = mx->w[x * 5 + y];
        mx->R[x] = Rx;
        if (Rx <= 0 || Rx <= worst) ok = 0;
        const int64_t loss = Rx - worst < Rx ? Rx - worst : Rx;
        if (loss < lam) lam = loss;
    }
    int64_t rn = 0;
    for (int y = 0; y < 5; y++) if (mx->w[20 + y] > rn) rn = mx->w[20 + y];
    mx->R[4] = rn;
    mx->lambda = lam;
    mx->ok = (ok && lam > 0) ? 1 : 0;
}

// Entry k = 8 x + y of the table with row stride 8 (the kernel's copy in LDS: an index without a multiply); y = 5 .. 7 is padding.
// k < 32: the rows of A C G T (the N-free rule's table); k < 40: with the N row.
GNX_CERT_HD inline int64_t gnx_cert_table8_entry(const GnxCertMatrix *mx, int k) { return (k & 7) < 5 ? mx->w[(k >> 3) * 5 + (k & 7)] : 0; }

// ---- a row ----
// Read base a against the window's bases on diagonal c (bd), on its first n columns (bf) and on its last n columns (bl):
// mid = w(a, bd), the row's loss on the diagonal R_a - mid, and what the row gains on the first / last columns instead.
// w = the table with row stride STRIDE (5: GnxCertMatrix::w, 8: gnx_cert_table8_entry).  Returns 0 for a byte >= 5, and for an N in the
// read unless allow_n: then the row's R is rn = R_N (the table needs its row 4).
struct GnxCertRow {
    int64_t mid, loss, f, g;
};
template <int STRIDE>
GNX_CERT_HD inline int gnx_certn_row(const int64_t *w, int64_t rn, int allow_n, unsigned a, unsigned bd, unsigned bf, unsigned bl, GnxCertRow *r) {
    if (a >= (allow_n ? 5u : 4u) || bd >= 5 || bf >= 5 || bl >= 5) return 0;
    const int64_t *wa = w + a * STRIDE;
    const int64_t mid = wa[bd];
    r->mid = mid; r->loss = (a < 4 ? wa[a] : rn) - mid; r->f = wa[bf] - mid; r->g = wa[bl] - mid;
    return 1;
}
template <int STRIDE>
GNX_CERT_HD inline int gnx_cert_row(const int64_t *w, unsigned a, unsigned bd, unsigned bf, unsigned bl, GnxCertRow *r) {
    return gnx_certn_row<STRIDE>(w, 0, 0, a, bd, bf, bl, r);
}

// ---- a lane's chunk of consecutive rows, taken in ascending order ----
// Sums of the four terms; f_top = the largest of the chunk's own prefix sums of f (item 6: the prefix before the chunk + f_top <= 0);
// g_low = the least sum of g over the chunk's rows BEFORE a row and g_row = the first row that attains it (the suffix sum G from
// that row on is the chunk's largest, and of equal ones the longest).  nn = the chunk's N rows (their sum over the lanes is nu).
struct GnxCertLane {
    int64_t loss, mid, f, g, f_top, g_low;
    int32_t g_row, rows, ok, nn;
};
GNX_CERT_HD inline void gnx_cert_lane_init(GnxCertLane *l) {
    l->loss = l->mid = l->f = l->g = l->f_top = l->g_low = 0;
    l->g_row = 0; l->rows = 0; l->ok = 1; l->nn = 0;
}
// row i joins the chunk; returns its loss (the edge rule's sums)
template <int STRIDE>
GNX_CERT_HD inline int64_t gnx_certn_lane_row(GnxCertLane *l, const int64_t *w, int64_t rn, int allow_n, int i, unsigned a, unsigned bd, unsigned bf,
                                              unsigned bl) {
    GnxCertRow r;
    if (!gnx_certn_row<STRIDE>(w, rn, allow_n, a, bd, bf, bl, &r)) { l->ok = 0; return 0; }
    l->nn += a == 4 ? 1 : 0;
    if (l->rows == 0 || l->g < l->g_low) { l->g_low = l->g; l->g_row = i; }
    l->loss += r.loss; l->mid += r.mid; l->f += r.f; l->g += r.g;
    if (l->rows == 0 || l->f > l->f_top) l->f_top = l->f;
    l->rows++;
    return r.loss;
}
template <int STRIDE>
GNX_CERT_HD inline int64_t gnx_cert_lane_row(GnxCertLane *l, const int64_t *w, int i, unsigned a, unsigned bd, unsigned bf, unsigned bl) {
    return gnx_certn_lane_row<STRIDE>(l, w, 0, 0, i, a, bd, bf, bl);
}
// (least prefix, first row) of two chunks
GNX_CERT_HD inline void gnx_cert_low_min(int64_t *low, int *row, int64_t other_low, int other_row) {
    if (other_low < *low || (other_low == *low && other_row < *row)) { *low = other_low; *row = other_row; }
}

// ---- the thresholds: items 4 and 5 from the deficit D ----
// ok = 0: refused.  edge = 1: -o < D < -2o, the edge rule decides: the loss of the first / last T1 and T2 rows (T1 + T2 < n).
struct GnxCertBounds {
    int64_t T1, T2;
    int32_t ok, edge;
};
// x / y for x >= 0 < y; values below 2^32, as every call of the kernel has them, take a 32-bit division
GNX_CERT_HD inline int64_t gnx_cert_div(int64_t x, int64_t y) {
    if ((((uint64_t)x | (uint64_t)y) >> 32) == 0) return (int64_t)((uint32_t)x / (uint32_t)y);
    return x / y;
}
// nu = the read's N rows: rows that cut exact runs like imperfect ones but lose >= 0, not >= lambda, so they stand beside J everywhere
GNX_CERT_HD inline GnxCertBounds gnx_certn_bounds(int64_t lambda, int64_t o, int64_t n, int64_t K, int64_t D, int64_t nu) {
    GnxCertBounds t = {0, 0, 0, 0};
    const int64_t O = -o;
    if (K > n) return t; // (every ceiling below is at most n)
    if (D == O || D >= 2 * O) return t; // (deficit == -o: a perfect path with three gap runs ties; refused, not argued)
    const int64_t J = gnx_cert_div(D, lambda) + nu, J1 = gnx_cert_div(D + O, lambda) + nu; // (with nu: rows that are not in an exact run)
    if (n - J <= 0 || n - J1 <= 0) return t;
    // K <= ceil(x / y)  <=>  (K - 1) y < x
    if ((K - 1) * (3 + J) >= n - J || (K - 1) * (2 + J1) >= n - J1) return t;
    if (D > O) {
        // -o < deficit < -2o: paths with three gap runs.  Off diagonal c they need an exact run of K rows (the third inequality); with a
        // segment on diagonal c they have to save -o or more on the rows outside it: at most T1 rows at one end and T2 at the other.
        const int64_t J3 = gnx_cert_div(D - O, lambda) + nu;
        if ((K - 1) * (4 + J3) >= n - J3) return t;
        t.T1 = (1 + J3) * (K - 1) + J3; t.T2 = (2 + J3) * (K - 1) + J3;
        if (t.T1 + t.T2 >= n) return t; // (every row is an edge row: E = deficit)
        t.edge = 1;
    }
    t.ok = 1;
    return t;
}
GNX_CERT_HD inline GnxCertBounds gnx_cert_bounds(int64_t lambda, int64_t o, int64_t n, int64_t K, int64_t D) {
    return gnx_certn_bounds(lambda, o, n, K, D, 0);
}

// ---- the tail: G_d = the sum of g over the last d rows, G_0 = 0; the LARGEST d that attains the maximum ----
// g_tot = the sum of g over all rows, (g_low, g_row) = the least sum of g over the rows before a row and the first row that attains it.
GNX_CERT_HD inline void gnx_cert_tail(int64_t g_tot, int64_t g_low, int64_t g_row, int64_t n, int64_t *best, int64_t *d_star) {
    const int64_t G = g_tot - g_low;
    if (G >= 0) { *best = G; *d_star = n - g_row; } else { *best = 0; *d_star = 0; }
}

// ---- the finishing arithmetic: items 4 (the edge rule's corners), 6 and the score ----
// f_pos: some F_alpha > 0; h1, h2 / t1, t2 = the loss of the first / last T1 and T2 rows (read only when t->edge).
GNX_CERT_HD inline int gnx_cert_finish(const GnxCertBounds *t, int64_t o, int64_t e, int64_t n, int64_t m, int f_pos, int64_t mid_sum, int64_t h1,
                                       int64_t h2, int64_t t1, int64_t t2, int64_t best, int64_t ds, int64_t *d_star, int64_t *score) {
    if (!t->ok || f_pos) return 0;
    if (t->edge && (h1 + t2 >= -o || h2 + t1 >= -o)) return 0;
    if (ds >= n) return 0;
    *d_star = ds;
    *score = mid_sum + best + 2 * o + e * (n + m);
    return 1;
}

// Items 1 (shape and checkerboard), 2 (no N in the read unless allow_n), 4, 5 and 6 of the certificate for a pair whose exact K-mer
// matches all lie on diagonal c (item 3, the caller's scan).  a[0..n) = the read; bd / bf / bl[0..n) = the window's bases under the read on
// diagonal c, on the window's first n columns and on its last n columns (b + c, b, b + m - n).  Item 4 has two branches: deficit < -o, or
// -o < deficit < -2o with the edge rule (a second pass over at most T2 rows from each end, running sums only).  Returns 1 and the
// closed form -- d* = the trailing read bases that sit on the window's last columns, the score -- or 0: the pair goes through the sweep.
// edge / nu (may be null): whether the edge rule decided, the read's N rows.  The serial composition of the pieces above.
GNX_CERT_HD inline int gnx_certn_decide(const GnxCertMatrix *mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl,
                                        int64_t m, int64_t c, int64_t K, int64_t ci, int64_t cj, int allow_n, int64_t *d_star, int64_t *score,
                                        int64_t *edge, int64_t *nu_out) {
    if (!mx->ok || n < 1 || K < 1 || m < n + 2 || c <= 0 || c >= m - n) return 0;
    if (ci < n || cj < m) return 0; // a checkerboard edge inside the matrix: quirks Q1 / Q2 are the walk's business
    const int64_t rn = mx->R[4];
    GnxCertRow r, r2;
    int64_t deficit = 0, mid_sum = 0, F = 0, nu = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!gnx_certn_row<5>(mx->w, rn, allow_n, a[i], bd[i], bf[i], bl[i], &r)) return 0;
        nu += a[i] == 4 ? 1 : 0;
        deficit += r.loss;
        mid_sum += r.mid;
        F += r.f; // the first i + 1 rows on the window's first columns instead (ties stay on the diagonal)
        if (F > 0) return 0;
    }
    const GnxCertBounds t = gnx_certn_bounds(mx->lambda, mx->o, n, K, deficit, nu);
    if (!t.ok) return 0;
    int64_t h1 = 0, h2 = 0, t1 = 0, t2 = 0; // the loss of the first / last T1 and T2 rows
    if (t.edge)
        for (int64_t i = 0; i < t.T2; i++) {
            const int64_t j = n - 1 - i;
            gnx_certn_row<5>(mx->w, rn, allow_n, a[i], bd[i], bf[i], bl[i], &r);
            gnx_certn_row<5>(mx->w, rn, allow_n, a[j], bd[j], bf[j], bl[j], &r2);
            h2 += r.loss; t2 += r2.loss;
            if (i < t.T1) { h1 += r.loss; t1 += r2.loss; }
        }
    int64_t G = 0, best = 0, ds = 0;
    for (int64_t d = 1; d <= n; d++) { // the last d rows on the window's last columns instead: the LARGEST d that attains the maximum
        const int64_t i = n - d;
        gnx_certn_row<5>(mx->w, rn, allow_n, a[i], bd[i], bf[i], bl[i], &r);
        G += r.g;
        if (G >= best) { best = G; ds = d; }
    }
    if (edge) *edge = t.edge;
    if (nu_out) *nu_out = nu;
    return gnx_cert_finish(&t, mx->o, mx->e, n, m, 0, mid_sum, h1, h2, t1, t2, best, ds, d_star, score);
}
GNX_CERT_HD inline int gnx_cert_decide(const GnxCertMatrix *mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl,
                                       int64_t m, int64_t c, int64_t K, int64_t ci, int64_t cj, int64_t *d_star, int64_t *score) {
    return gnx_certn_decide(mx, a, n, bd, bf, bl, m, c, K, ci, cj, 0, d_star, score, nullptr, nullptr);
}

// ---- the edge rule graded by the known end diagonals ("The edge rule on the known end diagonals") ----
// Applies where gnx_certn_bounds gave ok and edge, items 3 and 6 hold and a corner of gnx_cert_finish failed.  A three-run path that
// reaches diagonal c by its first run has the rows before that on diagonal 0, one that leaves c by its last run has the rows after it on
// diagonal m - n: both are loaded for item 6, so the real bytes bound those segments instead of "exact runs shorter than K".
// Row i is non-free on diagonal 0 (nf0) / m - n (nfm) when its read base is not N and differs from the window's byte there.
GNX_CERTE_HD inline void gnx_certe_flags(unsigned a, unsigned bf, unsigned bl, int *nf0, int *nfm) {
    *nf0 = (a != 4 && a != bf) ? 1 : 0;
    *nfm = (a != 4 && a != bl) ? 1 : 0;
}
// A lane's chunk of consecutive rows from row i0 on, taken in ascending order: bit k of bits0 / bitsm = row i0 + k is non-free.
struct GnxCertEdgeLane {
    int32_t bits0, bitsm, c0, cm, i0, rows;
};
GNX_CERTE_HD inline void gnx_certe_lane_init(GnxCertEdgeLane *l, int i0) { l->bits0 = l->bitsm = l->c0 = l->cm = 0; l->i0 = i0; l->rows = 0; }
GNX_CERTE_HD inline void gnx_certe_lane_row(GnxCertEdgeLane *l, unsigned a, unsigned bf, unsigned bl) {
    int f0, fm;
    gnx_certe_flags(a, bf, bl, &f0, &fm);
    l->bits0 |= f0 << l->rows; l->bitsm |= fm << l->rows;
    l->c0 += f0; l->cm += fm;
    l->rows++;
}
// The chunk's row that is the (j + 1)-th non-free one on diagonal 0 counted from row 0, when before0 = the non-free rows of the chunks
// before this one; -1: not in this chunk.  A0(j) = that row (the first A0 rows hold j non-free ones), n when no chunk has it.
GNX_CERTE_HD inline int gnx_certe_head_row(const GnxCertEdgeLane *l, int before0, int j) {
    int r = j - before0;
    if (r < 0 || r >= l->c0) return -1;
    for (int k = 0; k < l->rows; k++) if ((l->bits0 >> k) & 1) { if (r == 0) return l->i0 + k; r--; }
    return -1;
}
// The same from the read's end on diagonal m - n, afterm = the non-free rows of the chunks after this one; Am(j) = n - 1 - that row.
GNX_CERTE_HD inline int gnx_certe_tail_row(const GnxCertEdgeLane *l, int afterm, int j) {
    int r = j - afterm;
    if (r < 0 || r >= l->cm) return -1;
    for (int k = l->rows - 1; k >= 0; k--) if ((l->bitsm >> k) & 1) { if (r == 0) return l->i0 + k; r--; }
    return -1;
}
// The graded corners for j imperfect non-N rows outside the segment on diagonal c: rows before / after the segment of the two families
// (delta1 = c: pq[0], pq[1]; delta2 = c: pq[2], pq[3]).  Ts(J3) = T1 and Tt(J3) = T2 of gnx_certn_bounds.
GNX_CERTE_HD inline void gnx_certe_corners(int64_t K, int64_t nu, int64_t j, int64_t A0, int64_t Am, int64_t pq[4]) {
    const int64_t Ts = (1 + j + nu) * (K - 1) + j + nu, Tt = (2 + j + nu) * (K - 1) + j + nu;
    pq[0] = A0 < Ts ? A0 : Ts; pq[1] = Ts + Am < Tt ? Ts + Am : Tt;
    pq[2] = Ts + A0 < Tt ? Ts + A0 : Tt; pq[3] = Am < Ts ? Am : Ts;
}
// E(p, q) as two prefix sums of the loss: the rows [0, *head) and [*tail, n), E = P[*head] + D - P[*tail] with P[k] = the loss of the first k rows
GNX_CERTE_HD inline void gnx_certe_span(int64_t n, int64_t p, int64_t q, int64_t *head, int64_t *tail) {
    const int64_t pp = p < n ? p : n, qq = q < n - pp ? q : n - pp;
    *head = pp; *tail = n - qq;
}
// one grade: both corners strictly below O + lambda j
GNX_CERTE_HD inline int gnx_certe_grade(int64_t lambda, int64_t o, int64_t j, int64_t e1, int64_t e2) {
    const int64_t lim = -o + lambda * j;
    return (e1 < lim && e2 < lim) ? 1 : 0;
}
// the number of grades: j = 0 .. J3 without nu
GNX_CERTE_HD inline int64_t gnx_certe_grades(int64_t lambda, int64_t o, int64_t D) { return gnx_cert_div(D + o, lambda); }

// The serial decision: today's rule, then -- only where it fails at the corners -- the graded test.  by_edge (may be null) = 1 when the graded
// test admitted the pair and the old rule did not; jdec (may be null) = the largest grade at which the K-run bound alone (A0 = Am = n)
// would have refused, -1 when none (diagnostics: which grade the bytes decided).  Score and d* are the old rule's closed form.
GNX_CERT_HD inline int gnx_certe_decide(const GnxCertMatrix *mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl,
                                        int64_t m, int64_t c, int64_t K, int64_t ci, int64_t cj, int allow_n, int64_t *d_star, int64_t *score,
                                        int64_t *edge, int64_t *nu_out, int64_t *by_edge, int64_t *jdec) {
    if (by_edge) *by_edge = 0;
    if (jdec) *jdec = -1;
    if (gnx_certn_decide(mx, a, n, bd, bf, bl, m, c, K, ci, cj, allow_n, d_star, score, edge, nu_out)) return 1;
    if (!mx->ok || n < 1 || K < 1 || m < n + 2 || c <= 0 || c >= m - n || ci < n || cj < m) return 0;
    const int64_t rn = mx->R[4];
    GnxCertRow r;
    int64_t D = 0, mid_sum = 0, F = 0, nu = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!gnx_certn_row<5>(mx->w, rn, allow_n, a[i], bd[i], bf[i], bl[i], &r)) return 0;
        nu += a[i] == 4 ? 1 : 0;
        D += r.loss; mid_sum += r.mid; F += r.f;
        if (F > 0) return 0;
    }
    const GnxCertBounds t = gnx_certn_bounds(mx->lambda, mx->o, n, K, D, nu);
    if (!t.ok || !t.edge) return 0;
    int64_t G = 0, best = 0, ds = 0;
    for (int64_t d = 1; d <= n; d++) {
        gnx_certn_row<5>(mx->w, rn, allow_n, a[n - d], bd[n - d], bf[n - d], bl[n - d], &r);
        G += r.g;
        if (G >= best) { best = G; ds = d; }
    }
    if (ds >= n) return 0;
    // P[k] by a running sum: E of a corner walks its rows (serial: at most (1 + J3) corners of <= n rows)
    auto E = [&](int64_t p, int64_t q) -> int64_t {
        int64_t head, tail, s = 0;
        gnx_certe_span(n, p, q, &head, &tail);
        for (int64_t i = 0; i < n; i++)
            if (i < head || i >= tail) { gnx_certn_row<5>(mx->w, rn, allow_n, a[i], bd[i], bf[i], bl[i], &r); s += r.loss; }
        return s;
    };
    const int64_t J30 = gnx_certe_grades(mx->lambda, mx->o, D);
    for (int64_t j = 0; j <= J30; j++) {
        int64_t A0 = n, Am = n, seen = 0;
        int f0, fm;
        for (int64_t i = 0; i < n; i++) { gnx_certe_flags(a[i], bf[i], bl[i], &f0, &fm); if (f0 && seen++ == j) { A0 = i; break; } }
        seen = 0;
        for (int64_t i = n - 1; i >= 0; i--) { gnx_certe_flags(a[i], bf[i], bl[i], &f0, &fm); if (fm && seen++ == j) { Am = n - 1 - i; break; } }
        int64_t pq[4];
        gnx_certe_corners(K, nu, j, A0, Am, pq);
        if (!gnx_certe_grade(mx->lambda, mx->o, j, E(pq[0], pq[1]), E(pq[2], pq[3]))) return 0;
        if (jdec) {
            gnx_certe_corners(K, nu, j, n, n, pq);
            if (!gnx_certe_grade(mx->lambda, mx->o, j, E(pq[0], pq[1]), E(pq[2], pq[3]))) *jdec = j;
        }
    }
    *d_star = ds;
    *score = mid_sum + best + 2 * mx->o + mx->e * (n + m);
    if (edge) *edge = 1;
    if (nu_out) *nu_out = nu;
    if (by_edge) *by_edge = 1;
    return 1;
}

// Item 3 the naive way (host: the debug entry).  Exact K-mer matches of read positions q .. q + K - 1 and window positions j .. j + K - 1 over
// all q, j; window bytes that are not A C G T count as their two low bits, like in the kernel's rolling code (a false hit can only
// refuse).  A K-mer of the read that holds an N matches nothing: the N-aware rule's table leaves such K-mers out, so this is its scan too.
// Returns 1 and the diagonal when the matches are non-empty and share one diagonal c = j - q.
inline int gnx_cert_scan_naive(const uint8_t *a, int64_t n, const uint8_t *b, int64_t m, int64_t K, int64_t *c_out) {
    int found = 0;
    int64_t c = 0;
    for (int64_t q = 0; q + K <= n; q++)
        for (int64_t j = 0; j + K <= m; j++) {
            int64_t t = 0;
            while (t < K && a[q + t] < 4 && a[q + t] == (b[j + t] & 3)) t++;
            if (t < K) continue;
            if (found && j - q != c) return 0;
            found = 1; c = j - q;
        }
    *c_out = c;
    return found;
}
