// The gapless certificate's decision the way fp_cert_kernel evaluates it (gonomics_amd/csrc/fp_cert.hip.h), on
// the host: 64 emulated lanes, each with a contiguous chunk of ceil(n / 64) rows, the kernel's wave sums (xor butterfly), prefix scans
// (shift-up steps 1, 2, .. 32) and its (least prefix, first row) butterfly, built from the shared pieces of fp_cert_decide.h only.
// Every decision must equal gnx_cert_decide -- accept / refuse, d* and score -- on heap buffers of exactly n and m bytes, so that a
// sanitizer build (-fsanitize=address,undefined) sees every index.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../gonomics_amd/csrc/fp_cert_decide.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }

static const int64_t HCT[25] = {90, -330, -236, -356, -208, -330, 100, -318, -236, -196, -236, -318, 100, -330, -196,
                                -356, -236, -330, 90, -208, -208, -196, -196, -208, -202};

// ---- the wave ----------------------------------------------------------------------------------------------------------------------
static const int W = 64;

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

static int wave_decide(const GnxCertMatrix &mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl, int64_t m,
                       int64_t c, int64_t K, int64_t ci, int64_t cj, int64_t *d_star, int64_t *score) {
    // what the launch and the kernel's head decide: the matrix, the shape, the diagonal
    if (!mx.ok || n < 1 || n > 3 * W || K < 1 || m < n + 2 || c <= 0 || c >= m - n || ci < n || cj < m) return 0;
    int64_t w8[32];
    for (int k = 0; k < 32; k++) w8[k] = gnx_cert_table8_entry(&mx, k);
    const int chunk = (int)((n + W - 1) / W);
    GnxCertLane ln[W];
    int64_t loss[W][3];
    bool bad = false;
    for (int l = 0; l < W; l++) {
        gnx_cert_lane_init(&ln[l]);
        for (int k = 0; k < 3; k++) {
            const int64_t i = (int64_t)l * chunk + k;
            loss[l][k] = 0;
            if (k < chunk && i < n) loss[l][k] = gnx_cert_lane_row<8>(&ln[l], w8, (int)i, a[i], bd[i], bf[i], bl[i]);
        }
        if (!ln[l].ok) bad = true;
    }
    if (bad) return 0; // __any
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
    const GnxCertBounds t = gnx_cert_bounds(mx.lambda, mx.o, n, K, D[0]);
    int64_t h1[W], h2[W], t1[W], t2[W];
    for (int l = 0; l < W; l++) h1[l] = h2[l] = t1[l] = t2[l] = 0;
    if (t.edge) {
        for (int l = 0; l < W; l++)
            for (int k = 0; k < 3; k++) {
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
    return gnx_cert_finish(&t, mx.o, mx.e, n, m, f_pos, M[0], h1[0], h2[0], t1[0], t2[0], best, ds, d_star, score);
}

// ---- pairs -------------------------------------------------------------------------------------------------------------------------
struct Pair {
    std::vector<uint8_t> a, b;
    int64_t c;
};

// a random window of exactly m bytes, the read = its bases on diagonal c
static Pair make(int64_t n, int64_t m, int64_t c) {
    Pair p;
    p.a.resize(n); p.b.resize(m); p.c = c;
    for (auto &x : p.b) x = (uint8_t)below(4);
    for (int64_t i = 0; i < n; i++) p.a[i] = p.b[c + i];
    return p;
}
// read base x against window base y at row i of diagonal c
static void plant(Pair &p, int64_t i, int x, int y) { p.a[i] = (uint8_t)x; p.b[p.c + i] = (uint8_t)y; }
// three disjoint regions: the window's first n columns, the diagonal, its last n columns; the first and the last columns hold a
// mismatch under every read base (A against T, the worst of its row, so that a planted A-against-T row on the diagonal gains nothing)
static Pair make_apart(int64_t n) {
    Pair p = make(n, 3 * n + 30, n + 10);
    for (int64_t i = 0; i < n; i++) p.b[i] = p.b[2 * n + 30 + i] = (uint8_t)(p.a[i] == 0 ? 3 : (p.a[i] + 1) & 3);
    return p;
}
// an A-against-y mismatch at row i of the diagonal of a make_apart pair (T under it on the first and last columns)
static void mis(Pair &p, int64_t i, int y = 3) {
    const int64_t n = (int64_t)p.a.size();
    plant(p, i, 0, y);
    p.b[i] = p.b[2 * n + 30 + i] = 3;
}
// rows [0, hi) / the last L rows of the read copied under themselves onto the window's first / last columns
static void head_copy(Pair &p, int64_t hi) { for (int64_t i = 0; i < hi; i++) p.b[i] = p.a[i]; }
static void tail_copy(Pair &p, int64_t L) {
    const int64_t n = (int64_t)p.a.size(), m = (int64_t)p.b.size();
    for (int64_t i = n - L; i < n; i++) p.b[m - n + i] = p.a[i];
}

static int64_t decisions = 0, certified = 0, second = 0;

// both ways; returns the serial decision, d* through *ds_out
static int both(const GnxCertMatrix &mx, const Pair &p, int64_t K, int64_t *ds_out = nullptr, int64_t ci = -1, int64_t cj = -1) {
    const int64_t n = (int64_t)p.a.size(), m = (int64_t)p.b.size(), c = p.c;
    if (ci < 0) ci = n;
    if (cj < 0) cj = m;
    int64_t ds = -1, sc = -1, ds2 = -2, sc2 = -2;
    const int want = gnx_cert_decide(&mx, p.a.data(), n, p.b.data() + c, p.b.data(), p.b.data() + (m - n), m, c, K, ci, cj, &ds, &sc);
    const int got = wave_decide(mx, p.a.data(), n, p.b.data() + c, p.b.data(), p.b.data() + (m - n), m, c, K, ci, cj, &ds2, &sc2);
    CHECK(got == want);
    if (got && want) CHECK(ds == ds2 && sc == sc2);
    decisions++;
    if (want) {
        certified++;
        int64_t D = 0;
        for (int64_t i = 0; i < n; i++) D += mx.R[p.a[i]] - mx.w[p.a[i] * 5 + p.b[c + i]];
        if (D > -mx.o) second++;
        if (ds_out) *ds_out = ds;
    }
    return want;
}

static GnxCertMatrix matrix(const int64_t *scores, int64_t o, int64_t e) {
    GnxCertMatrix mx;
    gnx_cert_matrix_init(&mx, scores, o, e);
    return mx;
}

int main() {
    const int64_t pens[4][2] = {{-600, -150}, {-400, -30}, {-300, -150}, {-250, -150}};

    // ---- every n from 16 to 160, K from 1 to beyond n, random pairs ----
    for (int64_t n = 16; n <= 160; n++)
        for (int k = 0; k < 8; k++) {
            const GnxCertMatrix mx = matrix(HCT, pens[k % 4][0], pens[k % 4][1]);
            CHECK(mx.ok);
            const int64_t m = n + 2 + below(k % 3 ? 40 : 400), c = 1 + below(m - n - 1);
            Pair p = make(n, m, c);
            if (k == 5) p.b[below(m)] = 4;
            const int nm = (int)below(5);
            for (int t = 0; t < nm; t++) { // mismatches: at the head, at the tail, anywhere
                const int64_t e = below(n < 50 ? n : 50), q = t % 3 == 0 ? e : (t % 3 == 1 ? n - 1 - e : below(n));
                p.a[q] = (uint8_t)((p.a[q] + 1 + below(3)) & 3);
            }
            if (k == 6 && n % 8 == 1) p.a[below(n)] = 4;
            if (k % 4 == 2) { const int64_t L = 1 + below(12); for (int64_t i = 0; i < L; i++) p.b[i] = p.a[i]; }            // a head copy
            if (k % 4 == 3) { const int64_t L = 1 + below(12); for (int64_t i = 0; i < L; i++) p.b[m - L + i] = p.a[n - L + i]; } // a tail copy
            for (int64_t K : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)16, n / 3 + 1, n, n + 5}) both(mx, p, K);
            both(mx, p, 2, nullptr, n - 1, m); // a checkerboard edge inside the matrix
            both(mx, p, 2, nullptr, n, m - 1);
        }
    CHECK(certified >= 500);

    // ---- the deficit's boundaries: D = O - 1, O, O + 1, 2 O - 1, 2 O ----
    {
        int64_t odd[25];
        for (int x = 0; x < 25; x++) odd[x] = HCT[x];
        odd[1] = -331; // A against C loses 421, A against G 326
        Pair p = make_apart(150);
        mis(p, 70, 1); mis(p, 80, 2); // D = 747
        CHECK(both(matrix(odd, -748, -150), p, 16) == 1); // D = O - 1
        CHECK(both(matrix(odd, -747, -150), p, 16) == 0); // D = O
        CHECK(both(matrix(odd, -746, -150), p, 16) == 1); // D = O + 1
        CHECK(both(matrix(odd, -374, -150), p, 16) == 1); // D = 2 O - 1
        Pair q = make_apart(150);
        mis(q, 70, 2); mis(q, 80, 2); // D = 652
        CHECK(both(matrix(HCT, -326, -150), q, 16) == 0); // D = 2 O
        CHECK(both(matrix(HCT, -327, -150), q, 16) == 1);
        CHECK(both(matrix(HCT, -651, -150), q, 16) == 1); // D = O + 1
        CHECK(both(matrix(HCT, -652, -150), q, 16) == 0); // D = O
        CHECK(both(matrix(HCT, -653, -150), q, 16) == 1); // D = O - 1
    }

    // ---- the edge rule: HCT, O = 600, K = 16, two A-against-T mismatches (D = 892): J3 = 0, T1 = 15, T2 = 30 ----
    {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        const int refused[8][2] = {{3, 29}, {14, 29}, {120, 146}, {120, 135}, {14, 134}, {15, 135}, {14, 120}, {3, 120}};
        const int accepted[7][2] = {{20, 130}, {3, 30}, {119, 135}, {15, 119}, {30, 134}, {14, 119}, {30, 135}};
        for (auto &r : refused) { Pair p = make_apart(150); mis(p, r[0]); mis(p, r[1]); CHECK(both(mx, p, 16) == 0); }
        for (auto &r : accepted) { Pair p = make_apart(150); mis(p, r[0]); mis(p, r[1]); CHECK(both(mx, p, 16) == 1); }
        // the rows T1 - 1 / T1 and T2 - 1 / T2 from either end at other read lengths (other chunk sizes) and K
        for (int64_t n : {(int64_t)96, (int64_t)128, (int64_t)129, (int64_t)160})
            for (int64_t K : {(int64_t)9, (int64_t)13, (int64_t)16}) {
                const int64_t T1 = K - 1, T2 = 2 * (K - 1);
                const GnxCertBounds t = gnx_cert_bounds(mx.lambda, mx.o, n, K, 892); // (item 5 refuses some of these n, K)
                if (t.ok) CHECK(t.edge && t.T1 == T1 && t.T2 == T2);
                auto in12 = [&](int64_t r) { return r < T1 || r >= n - T2; }; // a row of E(T1, T2)
                auto in21 = [&](int64_t r) { return r < T2 || r >= n - T1; }; // a row of E(T2, T1)
                for (int64_t r1 : {T1 - 1, T1, n - T1 - 1, n - T1})
                    for (int64_t r2 : {T2 - 1, T2, n - T2 - 1, n - T2}) {
                        Pair p = make_apart(n);
                        mis(p, r1); mis(p, r2);
                        const bool corner = (in12(r1) && in12(r2)) || (in21(r1) && in21(r2)); // one corner holds both: 892 >= 600
                        CHECK(both(mx, p, K) == (t.ok && !corner ? 1 : 0));
                    }
            }
        // T1 + T2 >= n: item 5 keeps n above T1 + T2 whenever O < D < 2 O (then J1 >= J3 + 2 and (K - 1)(2 + J1) < n - J1), so no pair
        // reaches that line through the decision -- checked here over small values -- and the shortest reads item 5 admits only agree
        for (int64_t lam = 1; lam <= 10; lam++)
            for (int64_t O = 1; O <= 36; O++)
                for (int64_t D = O + 1; D < 2 * O; D++)
                    for (int64_t n = 1; n <= 48; n++)
                        for (int64_t K = 1; K <= n; K++) {
                            const GnxCertBounds t = gnx_cert_bounds(lam, -O, n, K, D);
                            if (t.ok) CHECK(t.edge && t.T1 + t.T2 < n);
                            else CHECK(t.T1 == 0 && t.T2 == 0); // (refused before T1 and T2 were formed)
                        }
        for (int64_t K = 1; K <= 8; K++)
            for (int64_t n = 16; n <= 60; n++) {
                Pair p = make(n, n + 40, 9);
                plant(p, 1, 0, 3); plant(p, n - 2, 0, 3);
                both(mx, p, K);
            }
    }

    // ---- F_alpha > 0 first at alpha = 1, 64, 65, 128, n ----
    for (int64_t n : {(int64_t)129, (int64_t)150, (int64_t)160}) {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        for (int64_t alpha : {(int64_t)1, (int64_t)64, (int64_t)65, (int64_t)128, n}) {
            Pair p = make_apart(n);
            mis(p, alpha - 1);
            CHECK(both(mx, p, 16) == 1); // one mismatch, nothing of the read on the window's first columns
            head_copy(p, alpha);         // rows 0 .. alpha - 1 match them: F = 0 up to row alpha - 2, F_alpha = the mismatch's loss
            CHECK(both(mx, p, 16) == 0);
            p.b[alpha - 1] = 3;          // ... all but the last: F stays <= 0
            CHECK(both(mx, p, 16) == 1);
        }
    }

    // ---- the tail: d* = 0, a tie at G = 0 over 0 .. L trailing rows, ties above 0 and across a dip, d* = n - 1 and n ----
    for (int64_t n : {(int64_t)64, (int64_t)65, (int64_t)128, (int64_t)129, (int64_t)150, (int64_t)160}) {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        int64_t ds = -1;
        Pair p = make_apart(n);
        CHECK(both(mx, p, 8, &ds) == 1 && ds == 0);
        for (int64_t L : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)4, (int64_t)63, (int64_t)64, n - 2, n - 1}) {
            if (L >= n) continue;
            Pair q = make_apart(n);
            tail_copy(q, L); // G_d = 0 for d = 0 .. L: the largest wins
            CHECK(both(mx, q, 8, &ds) == 1 && ds == L);
        }
        Pair q = make_apart(n);
        tail_copy(q, n); // the whole read on the window's last columns: d* = n
        CHECK(both(mx, q, 8) == 0);
        for (int64_t r : {n - 1, n - 10, n - 20}) { // a mismatch on the diagonal that the tail copy does not have: G = its loss for d = n - r .. 20
            Pair t = make_apart(n);
            mis(t, r);
            tail_copy(t, 20);
            CHECK(both(mx, t, 8, &ds) == 1 && ds == 20);
        }
        for (int64_t r : {n - 7, (int64_t)70, (int64_t)63, (int64_t)1}) { // G_d = 0 for d < n - r - 1, a dip of one A-against-T loss at row r + 1, back to 0 at row r: a tie across the dip
            if (r + 2 > n) continue;
            Pair u = make_apart(n);
            tail_copy(u, n - r);               // rows r .. n - 1 match the window's last columns, but:
            mis(u, r);
            u.b[2 * n + 30 + r] = 0;           // row r: the tail has the A that the diagonal has not (+446)
            u.a[r + 1] = u.b[u.c + r + 1] = 0; // row r + 1: an A on the diagonal
            u.b[2 * n + 30 + r + 1] = 3;       // against T on the tail (-446)
            CHECK(both(mx, u, 8, &ds) == 1 && ds == n - r);
        }
    }

    // ---- an N in the read, a byte >= 5 in each of the three window regions ----
    for (int64_t n : {(int64_t)66, (int64_t)150, (int64_t)160}) {
        const GnxCertMatrix mx = matrix(HCT, -600, -150);
        for (int64_t r : {(int64_t)0, (int64_t)63, (int64_t)64, n - 1}) {
            Pair p = make_apart(n);
            p.a[r] = 4;
            CHECK(both(mx, p, 8) == 0);
            Pair q = make_apart(n);
            q.b[q.c + r] = 4; // an N in the window is a mismatch like another
            q.b[r] = q.b[2 * n + 30 + r] = 4;
            CHECK(both(mx, q, 8) == 1);
            for (int64_t at : {r, q.c + r, 2 * n + 30 + r}) { // bf, bd, bl
                Pair z = make_apart(n);
                z.b[at] = (uint8_t)(5 + below(250));
                CHECK(both(mx, z, 8) == 0);
            }
        }
    }

    // ---- a matrix the certificate refuses ----
    {
        int64_t badm[25];
        for (int x = 0; x < 25; x++) badm[x] = HCT[x];
        badm[0] = -400; // A against A below A against C
        const GnxCertMatrix mx = matrix(badm, -600, -150);
        CHECK(!mx.ok);
        Pair p = make_apart(150);
        CHECK(both(matrix(HCT, -600, -150), p, 16) == 1);
        CHECK(both(mx, p, 16) == 0);
        const GnxCertMatrix pos = matrix(HCT, 0, -150); // gapOpen >= 0
        CHECK(!pos.ok && both(pos, p, 16) == 0);
    }

    printf("cert_wave_test: %lld decisions, %lld certified, %lld of them with deficit > -o, %d failures\n", (long long)decisions, (long long)certified,
           (long long)second, fails);
    CHECK(second >= 100);
    return fails ? 1 : 0;
}
