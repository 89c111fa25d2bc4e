// The gapless certificate's N-aware decision the way fp_cert_kernel evaluates it (gonomics_amd/csrc/fp_cert.hip.h, DESIGN.md section 4.22,
// "Reads that hold N"), on the host: 64 emulated lanes, each with a contiguous chunk of ceil(n / 64) rows, the kernel's wave sums (xor
// butterfly), prefix scans, its (least prefix, first row) butterfly and its count of the N rows (one ballot per row of a chunk), built
// from the shared gnx_certn_* pieces of fp_cert_decide.h only.  Every decision must equal gnx_certn_decide -- accept / refuse, d* and
// score -- and, on reads without N, the old gnx_cert_decide; reads with N must be refused by the old one.  Heap buffers of exactly n
// and m bytes, so that a sanitizer build (-fsanitize=address,undefined) sees every index.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../gonomics_amd/csrc/fp_cert_decide.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }

static const int64_t HCT[25] = {90, -330, -236, -356, -208, -330, 100, -318, -236, -196, -236, -318, 100, -330, -196,
                                -356, -236, -330, 90, -208, -208, -196, -196, -208, -202};

// ---- the wave ----------------------------------------------------------------------------------------------------------------------
static const int W = 64, CHUNK = 3;

static void wave_sum(int64_t v[W]) { // v += __shfl_xor(v, d) for d = 32, 16, .. 1
    for (int d = 32; d >= 1; d >>= 1) {
        int64_t t[W];
        for (int l = 0; l < W; l++) t[l] = v[l ^ d];
        for (int l = 0; l < W; l++) v[l] += t[l];
    }
}

static void wave_scan(int64_t v[W]) { // inclusive: if (lane >= d) v += __shfl_up(v, d) for d = 1, 2, .. 32
    for (int d = 1; d < W; d <<= 1) {
        int64_t t[W];
        for (int l = 0; l < W; l++) t[l] = l >= d ? v[l - d] : 0;
        for (int l = 0; l < W; l++) v[l] += t[l];
    }
}

static int wave_decide_n(const GnxCertMatrix &mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl, int64_t m,
                         int64_t c, int64_t K, int64_t ci, int64_t cj, int64_t *d_star, int64_t *score, int64_t *nu_out) {
    // what the launch and the kernel's head decide: the matrix, the shape, the diagonal
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
    if (bad) return 0; // __any
    int64_t nu = 0; // one ballot per row of a chunk, the set bits counted
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
    for (int l = 1; l < W; l++) CHECK(D[l] == D[0] && M[l] == M[0] && low[l] == low[0] && row[l] == row[0]); // uniform
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
    *nu_out = nu;
    return gnx_cert_finish(&t, mx.o, mx.e, n, m, f_pos, M[0], h1[0], h2[0], t1[0], t2[0], best, ds, d_star, score);
}

// ---- pairs -------------------------------------------------------------------------------------------------------------------------
struct Pair {
    std::vector<uint8_t> a, b;
    int64_t c;
};

// three disjoint regions of a window of exactly 3 n + 30 bytes: its first n columns, the diagonal c = n + 10, its last n columns; the
// first and the last columns hold a mismatch under every read base
static Pair make_apart(int64_t n) {
    Pair p;
    p.a.resize(n); p.b.resize(3 * n + 30); p.c = n + 10;
    for (auto &x : p.b) x = (uint8_t)below(4);
    for (int64_t i = 0; i < n; i++) p.a[i] = p.b[p.c + i];
    for (int64_t i = 0; i < n; i++) p.b[i] = p.b[2 * n + 30 + i] = (uint8_t)(p.a[i] == 0 ? 3 : (p.a[i] + 1) & 3);
    return p;
}
// an A-against-y mismatch at row i of the diagonal (T under it on the first and last columns)
static void mis(Pair &p, int64_t i, int y = 3) {
    const int64_t n = (int64_t)p.a.size();
    p.a[i] = 0; p.b[p.c + i] = (uint8_t)y;
    p.b[i] = p.b[2 * n + 30 + i] = 3;
}
// an N at row i of the read over window base y on the diagonal (0 .. 4)
static void put_n(Pair &p, int64_t i, int y) { p.a[i] = 4; p.b[p.c + i] = (uint8_t)y; }

static int64_t decisions = 0, cert_n = 0, cert_n_edge = 0, cert_free = 0;

// the three ways; returns the serial N-aware decision
static int all(const GnxCertMatrix &mx, const Pair &p, int64_t K, int64_t *nu_ret = nullptr, int64_t ci = -1, int64_t cj = -1) {
    const int64_t n = (int64_t)p.a.size(), m = (int64_t)p.b.size(), c = p.c;
    if (ci < 0) ci = n;
    if (cj < 0) cj = m;
    const uint8_t *a = p.a.data(), *bd = p.b.data() + c, *bf = p.b.data(), *bl = p.b.data() + (m - n);
    int64_t ds = -1, sc = -1, ds2 = -2, sc2 = -2, ds3 = -3, sc3 = -3, edge = -1, nu = -1, nu2 = -2;
    const int want = gnx_certn_decide(&mx, a, n, bd, bf, bl, m, c, K, ci, cj, 1, &ds, &sc, &edge, &nu);
    const int got = wave_decide_n(mx, a, n, bd, bf, bl, m, c, K, ci, cj, &ds2, &sc2, &nu2);
    const int old = gnx_cert_decide(&mx, a, n, bd, bf, bl, m, c, K, ci, cj, &ds3, &sc3);
    CHECK(got == want);
    if (got && want) CHECK(ds == ds2 && sc == sc2 && nu == nu2);
    int64_t count = 0;
    for (int64_t i = 0; i < n; i++) count += p.a[i] == 4;
    if (want) CHECK(nu == count);
    if (count == 0) { // the N-free rule, unchanged
        CHECK(old == want);
        if (old && want) CHECK(ds == ds3 && sc == sc3);
    } else {
        CHECK(old == 0);
    }
    decisions++;
    if (want) { if (count) { cert_n++; cert_n_edge += edge; } else cert_free++; }
    if (nu_ret) *nu_ret = nu;
    return want;
}

static GnxCertMatrix matrix(const int64_t *scores, int64_t o, int64_t e) {
    GnxCertMatrix mx;
    gnx_cert_matrix_init(&mx, scores, o, e);
    return mx;
}

int main() {
    const int64_t pens[4][2] = {{-600, -150}, {-400, -30}, {-300, -150}, {-250, -150}};
    {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        CHECK(mx.ok && mx.R[4] == 104 && mx.R[4] - mx.w[24] == 6 && mx.lambda == 296);
        CHECK(matrix(HCT, -600, -30).R[4] == 0); // the N row below 0 after rebasing
    }

    // ---- every n from 16 to 160: N on the rows at the lane chunks' boundaries, over every window byte, both deficit branches ----
    for (int64_t n = 16; n <= 160; n++) {
        const int64_t chunk = (n + W - 1) / W;
        for (int64_t r : {(int64_t)0, (int64_t)63, (int64_t)64, (int64_t)127, (int64_t)128, n - 1, chunk, 2 * chunk - 1, 63 * chunk})
            for (int k = 0; k < 6; k++) {
                if (r >= n) continue;
                const GnxCertMatrix mx = matrix(HCT, pens[k % 4][0], pens[k % 4][1]);
                Pair p = make_apart(n);
                const int nm = k % 3; // 0, 1 or 2 mismatches: D < O and O < D < 2 O with HCT / -600
                for (int t = 0; t < nm; t++) { int64_t q = below(n); if (q != r) mis(p, q, 1 + (int)below(3)); }
                put_n(p, r, (int)below(5));
                if (k >= 3) { const int64_t q = below(n); put_n(p, q, (int)below(5)); } // a second N anywhere (or the same row)
                if (k == 5 && r + 1 < n) put_n(p, r + 1, 4);                              // ... and a third beside the first
                for (int64_t K : {(int64_t)1, (int64_t)4, (int64_t)9, (int64_t)16, n / 4 + 1, n + 1}) all(mx, p, K);
                all(mx, p, 2, nullptr, n - 1, -1); // a checkerboard edge inside the matrix
                p.b[below((int64_t)p.b.size())] = 7; // a byte >= 5 somewhere in the window
                all(mx, p, 4);
            }
        // reads without N: the old decision, the same results
        for (int k = 0; k < 4; k++) {
            const GnxCertMatrix mx = matrix(HCT, pens[k][0], pens[k][1]);
            Pair p = make_apart(n);
            for (int t = 0; t < k % 3; t++) mis(p, below(n), 1 + (int)below(3));
            for (int64_t K : {(int64_t)1, (int64_t)5, (int64_t)16, n}) all(mx, p, K);
        }
    }
    CHECK(cert_n >= 2000 && cert_n_edge >= 200 && cert_free >= 500);

    // ---- the deficit's boundaries with an N: two A-against-G mismatches and N over N, D = 2 x 326 + 6 = 658 ----
    {
        Pair p = make_apart(150);
        mis(p, 70, 2); mis(p, 80, 2); put_n(p, 40, 4);
        CHECK(all(matrix(HCT, -659, -150), p, 16) == 1); // D = O - 1
        CHECK(all(matrix(HCT, -658, -150), p, 16) == 0); // D = O
        CHECK(all(matrix(HCT, -657, -150), p, 16) == 1); // D = O + 1
        CHECK(all(matrix(HCT, -330, -150), p, 16) == 1); // D = 2 O - 2
        CHECK(all(matrix(HCT, -329, -150), p, 16) == 0); // D = 2 O
    }

    // ---- the edge rule with nu = 1: HCT, O = 600, two A-against-T mismatches (D = 892), an N over C: T1 = 2 (K - 1) + 1, T2 = 3 (K - 1) + 1 ----
    {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        for (int64_t n : {(int64_t)128, (int64_t)129, (int64_t)150, (int64_t)160})
            for (int64_t K : {(int64_t)9, (int64_t)13, (int64_t)16}) {
                const int64_t T1 = 2 * (K - 1) + 1, T2 = 3 * (K - 1) + 1;
                const GnxCertBounds t = gnx_certn_bounds(mx.lambda, mx.o, n, K, 892, 1);
                if (t.ok) CHECK(t.edge && t.T1 == T1 && t.T2 == T2);
                auto in12 = [&](int64_t r) { return r < T1 || r >= n - T2; }; // a row of E(T1, T2)
                auto in21 = [&](int64_t r) { return r < T2 || r >= n - T1; }; // a row of E(T2, T1)
                for (int64_t r1 : {T1 - 1, T1, n - T1 - 1, n - T1})
                    for (int64_t r2 : {T2 - 1, T2, n - T2 - 1, n - T2}) {
                        if (r1 == r2) continue;
                        Pair p = make_apart(n);
                        mis(p, r1); mis(p, r2);
                        int64_t rn = n / 2;
                        while (rn == r1 || rn == r2) rn++;
                        put_n(p, rn, 1);
                        const bool corner = (in12(r1) && in12(r2)) || (in21(r1) && in21(r2)); // one corner holds both: 892 >= 600
                        CHECK(all(mx, p, K) == (t.ok && !corner ? 1 : 0));
                    }
            }
        // a decision that passes has T1 + T2 < n.  (With nu > 0 item 5 no longer implies it -- J1 + nu >= J3 + nu + 2 is all that is left of
        // J1 >= 3 J3 -- so that line of the bounds does refuse here, which the corners would do as well: E = D >= O.)
        for (int64_t lam = 1; lam <= 8; lam++)
            for (int64_t O = 1; O <= 24; O++)
                for (int64_t D = O + 1; D < 2 * O; D++)
                    for (int64_t n = 1; n <= 40; n++)
                        for (int64_t K = 1; K <= n; K++)
                            for (int64_t nu = 0; nu <= 4; nu++) {
                                const GnxCertBounds t = gnx_certn_bounds(lam, -O, n, K, D, nu);
                                if (t.ok) CHECK(t.edge && t.T1 + t.T2 < n);
                                else if (nu == 0) CHECK(t.T1 == 0 && t.T2 == 0); // (N-free: refused before T1 and T2 were formed)
                            }
    }

    // ---- the most N item 5 admits at n = 150, K = 16 (N over C loses nothing: D = 0, J1 = 2): 5, and one more ----
    {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        const int64_t rows[6] = {20, 45, 70, 95, 120, 140};
        for (int cnt = 1; cnt <= 6; cnt++) {
            Pair p = make_apart(150);
            for (int t = 0; t < cnt; t++) put_n(p, rows[t], 1);
            int64_t nu = -1;
            CHECK(all(mx, p, 16, &nu) == (cnt <= 5 ? 1 : 0));
            if (cnt <= 5) CHECK(nu == cnt);
        }
    }

    // ---- N rows in the anchors: an N row's f and g come from the N row of the table ----
    {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        Pair p = make_apart(150);
        put_n(p, 0, 0);   // N over A on the diagonal (92), over C on the window's first column (104): F_1 = 12 > 0
        p.b[0] = 1;
        CHECK(all(mx, p, 16) == 0);
        p.b[0] = 0;       // ... over A there as well: F_1 = 0, a tie stays on the diagonal
        CHECK(all(mx, p, 16) == 1);
        Pair q = make_apart(150);
        put_n(q, 149, 0); // the last row: N over A on the diagonal, over C on the window's last column: G_1 = 12, d* = 1
        q.b[q.b.size() - 1] = 1;
        int64_t ds = -1, sc = -1;
        CHECK(all(mx, q, 16) == 1);
        CHECK(gnx_certn_decide(&mx, q.a.data(), 150, q.b.data() + q.c, q.b.data(), q.b.data() + 330, 480, q.c, 16, 150, 480, 1, &ds, &sc, nullptr, nullptr) == 1 && ds == 1);
    }

    printf("cert_n_test: %lld decisions, %lld certified with N (%lld by the edge rule), %lld without, %d failures\n", (long long)decisions,
           (long long)cert_n, (long long)cert_n_edge, (long long)cert_free, fails);
    return fails ? 1 : 0;
}
