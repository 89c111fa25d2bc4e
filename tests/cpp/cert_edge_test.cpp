// The edge rule graded by the known end diagonals the way fp_cert_kernel evaluates it (gonomics_amd/csrc/fp_cert.hip.h, DESIGN.md section
// 4.22, "The edge rule on the known end diagonals"), on the host: 64 emulated lanes, each with a contiguous chunk of ceil(n / 64) rows.  The
// older decision runs as in tests/cpp/cert_n_test.cpp; where it fails at the corners and nowhere else the lanes' non-free counts are scanned,
// the lane that holds the (j + 1)-th non-free row answers a ballot, and E comes from a prefix scan of the chunks' losses read from the lane
// of a row -- built from the shared gnx_certe_* pieces only.  Every decision must equal the serial gnx_certe_decide: accept / refuse, d*,
// score, and which rule admitted.  Heap buffers of exactly n and m bytes, so that a sanitizer build (-fsanitize=address,undefined) sees
// every index.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../gonomics_amd/csrc/fp_cert_decide.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }

static const int64_t HCT[25] = {90, -330, -236, -356, -208, -330, 100, -318, -236, -196, -236, -318, 100, -330, -196,
                                -356, -236, -330, 90, -208, -208, -196, -196, -208, -202};

static const int W = 64, CHUNK = 3;

static void wave_sum(int64_t v[W]) {
    for (int d = 32; d >= 1; d >>= 1) {
        int64_t t[W];
        for (int l = 0; l < W; l++) t[l] = v[l ^ d];
        for (int l = 0; l < W; l++) v[l] += t[l];
    }
}
static void wave_scan(int64_t v[W]) {
    for (int d = 1; d < W; d <<= 1) {
        int64_t t[W];
        for (int l = 0; l < W; l++) t[l] = l >= d ? v[l - d] : 0;
        for (int l = 0; l < W; l++) v[l] += t[l];
    }
}

static int max_grade = -1, graded_accepts = 0, graded_refusals = 0;

// by_edge: the graded test admitted
static int wave_decide_edge(const GnxCertMatrix &mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl, int64_t m,
                            int64_t c, int64_t K, int64_t ci, int64_t cj, int64_t *d_star, int64_t *score, int64_t *by_edge) {
    *by_edge = 0;
    if (!mx.ok || n < 1 || n > CHUNK * W || K < 1 || m < n + 2 || c <= 0 || c >= m - n || ci < n || cj < m) return 0;
    int64_t w8[40];
    for (int k = 0; k < 40; k++) w8[k] = gnx_cert_table8_entry(&mx, k);
    const int chunk = (int)((n + W - 1) / W);
    GnxCertLane ln[W];
    int64_t loss[W][CHUNK];
    bool bad = false;
    for (int l = 0; l < W; l++) {
        gnx_cert_lane_init(&ln[l]);
        for (int k = 0; k < CHUNK; k++) {
            const int64_t i = (int64_t)l * chunk + k;
            loss[l][k] = 0;
            if (k < chunk && i < n) loss[l][k] = gnx_certn_lane_row<8>(&ln[l], w8, mx.R[4], 1, (int)i, a[i], bd[i], bf[i], bl[i]);
        }
        if (!ln[l].ok) bad = true;
    }
    if (bad) return 0;
    int64_t nu = 0;
    for (int k = 0; k < CHUNK; k++)
        for (int l = 0; l < W; l++) nu += ln[l].nn > k ? 1 : 0;
    int64_t D[W], M[W], F[W], G[W], low[W];
    int row[W];
    for (int l = 0; l < W; l++) { D[l] = ln[l].loss; M[l] = ln[l].mid; F[l] = ln[l].f; G[l] = ln[l].g; }
    wave_sum(D); wave_sum(M); wave_scan(F); wave_scan(G);
    bool f_pos = false;
    for (int l = 0; l < W; l++) {
        if (ln[l].rows > 0 && F[l] - ln[l].f + ln[l].f_top > 0) f_pos = true;
        low[l] = ln[l].rows > 0 ? G[l] - ln[l].g + ln[l].g_low : INT64_MAX;
        row[l] = ln[l].rows > 0 ? ln[l].g_row : (int)n;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        int64_t tl[W];
        int tr[W];
        for (int l = 0; l < W; l++) { tl[l] = low[l ^ d]; tr[l] = row[l ^ d]; }
        for (int l = 0; l < W; l++) gnx_cert_low_min(&low[l], &row[l], tl[l], tr[l]);
    }
    const GnxCertBounds t = gnx_certn_bounds(mx.lambda, mx.o, n, K, D[0], nu);
    int64_t h1[W], h2[W], t1[W], t2[W];
    for (int l = 0; l < W; l++) h1[l] = h2[l] = t1[l] = t2[l] = 0;
    if (t.edge) {
        for (int l = 0; l < W; l++)
            for (int k = 0; k < CHUNK; k++) {
                const int64_t i = (int64_t)l * chunk + k;
                if (i < t.T1) h1[l] += loss[l][k];
                if (i < t.T2) h2[l] += loss[l][k];
                if (i >= n - t.T1) t1[l] += loss[l][k];
                if (i >= n - t.T2) t2[l] += loss[l][k];
            }
        wave_sum(h1); wave_sum(h2); wave_sum(t1); wave_sum(t2);
    }
    int64_t best, ds;
    gnx_cert_tail(G[W - 1], low[0], row[0], n, &best, &ds);
    if (gnx_cert_finish(&t, mx.o, mx.e, n, m, f_pos, M[0], h1[0], h2[0], t1[0], t2[0], best, ds, d_star, score)) return 1;
    // refused for the corners and for nothing else?
    if (!(t.ok && !f_pos && t.edge && ds < n && (h1[0] + t2[0] >= -mx.o || h2[0] + t1[0] >= -mx.o))) return 0;
    GnxCertEdgeLane el[W];
    int64_t inc0[W], incm[W], k0[W];
    for (int l = 0; l < W; l++) {
        gnx_certe_lane_init(&el[l], l * chunk);
        for (int k = 0; k < CHUNK; k++) {
            const int64_t i = (int64_t)l * chunk + k;
            if (k < chunk && i < n) gnx_certe_lane_row(&el[l], a[i], bf[i], bl[i]);
        }
        inc0[l] = el[l].c0; incm[l] = el[l].cm; k0[l] = ln[l].loss;
    }
    wave_scan(inc0); wave_scan(incm); wave_scan(k0);
    for (int l = 0; l < W; l++) k0[l] -= ln[l].loss;
    auto prefix = [&](int64_t k) -> int64_t { // the lane of row k answers
        if (k >= n) return D[0];
        const int L = (int)(k / chunk), r = (int)(k - (int64_t)L * chunk);
        CHECK(L < W);
        int64_t v = k0[L];
        for (int x = 0; x + 1 < CHUNK; x++) v += r > x ? loss[L][x] : 0;
        return v;
    };
    const int64_t J30 = gnx_certe_grades(mx.lambda, mx.o, D[0]);
    for (int64_t j = 0; j <= J30; j++) {
        int64_t A0 = n, Am = n;
        int holders0 = 0, holdersm = 0;
        for (int l = 0; l < W; l++) { // the ballots: one lane at most holds the row
            const int hr = gnx_certe_head_row(&el[l], (int)(inc0[l] - el[l].c0), (int)j), tr = gnx_certe_tail_row(&el[l], (int)(incm[W - 1] - incm[l]), (int)j);
            if (hr >= 0) { holders0++; A0 = hr; }
            if (tr >= 0) { holdersm++; Am = n - 1 - tr; }
        }
        CHECK(holders0 <= 1 && holdersm <= 1);
        int64_t pq[4], ha, ta, hb, tb;
        gnx_certe_corners(K, nu, j, A0, Am, pq);
        gnx_certe_span(n, pq[0], pq[1], &ha, &ta);
        gnx_certe_span(n, pq[2], pq[3], &hb, &tb);
        if (!gnx_certe_grade(mx.lambda, mx.o, j, prefix(ha) + D[0] - prefix(ta), prefix(hb) + D[0] - prefix(tb))) { graded_refusals++; return 0; }
        if (j > max_grade) max_grade = (int)j;
    }
    *d_star = ds;
    *score = M[0] + best + 2 * mx.o + mx.e * (n + m);
    *by_edge = 1;
    graded_accepts++;
    return 1;
}

// ---- pairs -------------------------------------------------------------------------------------------------------------------------
struct Pair {
    std::vector<uint8_t> a, b;
    int64_t c;
};
// three disjoint regions of a window of exactly 3 n + 30 bytes: its first n columns, the diagonal c = n + 10, its last n columns; the first
// and the last columns are copies of the read (every row free on both end diagonals)
static Pair make_free(int64_t n) {
    Pair p;
    p.a.resize(n); p.b.resize(3 * n + 30); p.c = n + 10;
    for (auto &x : p.b) x = (uint8_t)below(4);
    for (int64_t i = 0; i < n; i++) p.a[i] = p.b[p.c + i];
    for (int64_t i = 0; i < n; i++) p.b[i] = p.b[2 * n + 30 + i] = p.a[i];
    return p;
}
static uint8_t other(uint8_t x) { return (uint8_t)((x + 1 + below(3)) & 3); }
// row i non-free on diagonal 0 (side 0) or m - n (side 1): a mismatch there, so f or g of the row is negative
static void non_free(Pair &p, int64_t i, int side) {
    const int64_t n = (int64_t)p.a.size();
    if (p.a[i] >= 4) return;
    p.b[side == 0 ? i : 2 * n + 30 + i] = other(p.a[i]);
}
// a mismatch at row i of diagonal c; the end diagonals keep the window's base of diagonal c there (f = g = 0, non-free on both)
static void mis(Pair &p, int64_t i, int transition) {
    const int64_t n = (int64_t)p.a.size();
    const uint8_t y = p.b[p.c + i];
    p.a[i] = transition ? (uint8_t)(y ^ 2) : other(y);
    p.b[i] = p.b[2 * n + 30 + i] = y;
}

static int checked = 0, both_refuse = 0;
static void compare(const GnxCertMatrix &mx, const Pair &p, int64_t K) {
    const int64_t n = (int64_t)p.a.size(), m = (int64_t)p.b.size();
    const uint8_t *a = p.a.data(), *b = p.b.data();
    int64_t d1 = -1, s1 = -1, e1 = 0, d2 = -1, s2 = -1, e2 = 0, edge = 0, nu = 0, jdec = 0;
    const int r1 = gnx_certe_decide(&mx, a, n, b + p.c, b, b + (m - n), m, p.c, K, 10000, 10000, 1, &d1, &s1, &edge, &nu, &e1, &jdec);
    const int r2 = wave_decide_edge(mx, a, n, b + p.c, b, b + (m - n), m, p.c, K, 10000, 10000, &d2, &s2, &e2);
    CHECK(r1 == r2);
    if (r1 && r2) CHECK(d1 == d2 && s1 == s2 && e1 == e2);
    if (r1 && !e1) { // what the older serial decision admits it admits identically
        int64_t d3 = -1, s3 = -1;
        CHECK(gnx_certn_decide(&mx, a, n, b + p.c, b, b + (m - n), m, p.c, K, 10000, 10000, 1, &d3, &s3, nullptr, nullptr) && d3 == d1 && s3 == s1);
    }
    checked++;
    both_refuse += !r1;
}

int main() {
    GnxCertMatrix hct, low;
    gnx_cert_matrix_init(&hct, HCT, -600, -150);
    int64_t LOW[25];
    for (int k = 0; k < 25; k++) LOW[k] = HCT[k];
    LOW[0 * 5 + 2] = LOW[2 * 5 + 0] = LOW[1 * 5 + 3] = LOW[3 * 5 + 1] = 20; // transitions lose 70 or 80: lambda = 70, many grades under one gap open
    gnx_cert_matrix_init(&low, LOW, -600, -150);
    CHECK(hct.ok && hct.lambda == 296 && low.ok && low.lambda == 70);
    for (int64_t n = 16; n <= 160; n++) {
        const int chunk = (int)((n + W - 1) / W);
        for (int rep = 0; rep < 60; rep++) {
            const bool use_low = rep % 3 == 2;
            const GnxCertMatrix &mx = use_low ? low : hct;
            Pair p = make_free(n);
            const int tail = rep & 1;
            // mismatches near one end: with the low matrix as many transitions as put D between one and two gap opens
            const int nm = use_low ? 8 + (int)below(8) : 2 + (int)below(2);
            const int64_t span = n < 50 ? n : 45;
            for (int x = 0; x < nm; x++) { const int64_t q = below(span); mis(p, tail ? n - 1 - q : q, use_low || below(4) != 0); }
            // non-free rows: on both sides of a lane border, on rows 0 and n - 1, and at random with a density per pair
            const int64_t L = 1 + below((n + chunk - 1) / chunk - 1 > 0 ? (n + chunk - 1) / chunk - 1 : 1);
            const int mode = rep % 5;
            if (mode == 0) { non_free(p, 0, 0); non_free(p, n - 1, 1); }
            if (mode == 1 && L * chunk < n) { non_free(p, L * chunk - 1, 0); non_free(p, L * chunk, 0); non_free(p, L * chunk - 1, 1); non_free(p, L * chunk, 1); }
            if (mode == 2 && L * chunk < n) { non_free(p, L * chunk - 1, tail); non_free(p, n - 1 - (L * chunk - 1), 1 - tail); }
            if (mode == 3 && L * chunk < n) { non_free(p, L * chunk, tail); non_free(p, 0, 1); non_free(p, n - 1, 0); }
            const int dens = (int)below(4); // 0: none, then one row in 16, 6, 2
            for (int64_t i = 0; i < n && dens; i++)
                for (int side = 0; side < 2; side++) if (below(dens == 1 ? 16 : (dens == 2 ? 6 : 2)) == 0) non_free(p, i, side);
            if (rep % 7 == 6) p.a[below(n)] = 4; // an N row: free on both end diagonals, one more in nu
            for (int64_t K = use_low ? 2 : 6; K <= 16; K += use_low ? 1 : 5) compare(mx, p, K);
        }
    }
    printf("%d decisions, %d refused by both, %d admitted by the graded test, %d refused by it, grades up to j = %d\n", checked, both_refuse,
           graded_accepts, graded_refusals, max_grade);
    CHECK(graded_accepts >= 500 && graded_refusals >= 500 && max_grade >= 7); // (the generator is seeded: these are its figures' floor)
    printf("cert_edge_test: %d failures\n", fails);
    return fails ? 1 : 0;
}
