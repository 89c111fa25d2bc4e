// The gapless certificate's decision arithmetic (gonomics_amd/csrc/fp_cert_decide.h) as a stand-alone host program: a few thousand
// pairs through gnx_cert_scan_naive + gnx_cert_decide on heap buffers of exactly n and m bytes, so that a sanitizer build
// (-fsanitize=address,undefined) sees every index of the edge rule's second pass, K from 1 to beyond n included.  Each decision is
// compared with a restatement that keeps the per-row losses in an array and sums E(p, q) as section 4.22 defines it.
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

// E(p, q): the loss of the first min(p, n) rows and of the last min(q, n - p) rows, no row twice
static int64_t edge_loss(const std::vector<int64_t> &loss, int64_t p, int64_t q) {
    const int64_t n = (int64_t)loss.size();
    if (p > n) p = n;
    if (q > n - p) q = n - p;
    int64_t s = 0;
    for (int64_t i = 0; i < p; i++) s += loss[i];
    for (int64_t i = n - q; i < n; i++) s += loss[i];
    return s;
}

static int64_t ceil_div(int64_t x, int64_t y) { return (x + y - 1) / y; }

// items 2, 4, 5 and 6 restated (item 1 is the caller's here: 0 < c < m - n, no checkerboard)
static int restated(const GnxCertMatrix &mx, const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, int64_t c, int64_t K, int64_t *d_star, int64_t *score) {
    const int64_t n = (int64_t)a.size(), m = (int64_t)b.size(), O = -mx.o;
    std::vector<int64_t> loss(n);
    int64_t D = 0, mid = 0, F = 0;
    for (int64_t i = 0; i < n; i++) if (a[i] >= 4) return 0;
    for (int64_t i = 0; i < n; i++) {
        loss[i] = mx.R[a[i]] - mx.w[a[i] * 5 + b[c + i]];
        D += loss[i]; mid += mx.w[a[i] * 5 + b[c + i]];
        F += mx.w[a[i] * 5 + b[i]] - mx.w[a[i] * 5 + b[c + i]];
        if (F > 0) return 0;
    }
    if (D == O || D >= 2 * O) return 0;
    const int64_t J = D / mx.lambda, J1 = (D + O) / mx.lambda;
    if (n - J <= 0 || n - J1 <= 0 || K > ceil_div(n - J, 3 + J) || K > ceil_div(n - J1, 2 + J1)) return 0;
    if (D > O) {
        const int64_t J3 = (D - O) / mx.lambda, T1 = (1 + J3) * (K - 1) + J3, T2 = (2 + J3) * (K - 1) + J3;
        if (K > ceil_div(n - J3, 4 + J3)) return 0;
        if (edge_loss(loss, T1, T2) >= O || edge_loss(loss, T2, T1) >= O) return 0;
    }
    int64_t G = 0, best = 0, ds = 0;
    for (int64_t d = 1; d <= n; d++) {
        const int64_t i = n - d;
        G += mx.w[a[i] * 5 + b[m - n + i]] - mx.w[a[i] * 5 + b[c + i]];
        if (G >= best) { best = G; ds = d; }
    }
    if (ds >= n) return 0;
    *d_star = ds; *score = mid + best + 2 * mx.o + mx.e * (n + m);
    return 1;
}

int main() {
    const int64_t pens[4][2] = {{-600, -150}, {-400, -30}, {-300, -150}, {-250, -150}};
    int64_t certified = 0, second = 0, calls = 0;
    for (int k = 0; k < 4000; k++) {
        GnxCertMatrix mx;
        gnx_cert_matrix_init(&mx, HCT, pens[k % 4][0], pens[k % 4][1]);
        CHECK(mx.ok);
        const int64_t n = 16 + below(145), m = n + 2 + below(k % 3 ? 40 : 200), c = 1 + below(m - n - 1);
        std::vector<uint8_t> b(m), a(n);
        for (auto &x : b) x = (uint8_t)below(4);
        if (k % 16 == 5) b[below(m)] = 4;
        for (int64_t i = 0; i < n; i++) a[i] = b[c + i] & 3;
        const int nm = (int)below(5);
        for (int t = 0; t < nm; t++) { // mismatches: at the head, at the tail, anywhere
            const int64_t e = below(n < 50 ? n : 50), q = t % 3 == 0 ? e : (t % 3 == 1 ? n - 1 - e : below(n));
            a[q] = (uint8_t)((a[q] + 1 + below(3)) & 3);
        }
        if (k % 32 == 9) a[below(n)] = 4;
        if (k % 4 == 2) { const int64_t L = 1 + below(12); for (int64_t i = 0; i < L; i++) b[i] = a[i]; }            // a head copy
        if (k % 4 == 3) { const int64_t L = 1 + below(12); for (int64_t i = 0; i < L; i++) b[m - L + i] = a[n - L + i]; } // a tail copy
        const int64_t Ks[7] = {1, 2, 5, 16, n / 3 + 1, n, n + 5};
        for (int64_t K : Ks) {
            // the decision on diagonal c whatever a scan would say: every K reaches the arithmetic
            int64_t ds = -1, sc = -1, ds2 = -2, sc2 = -2;
            const int got = gnx_cert_decide(&mx, a.data(), n, b.data() + c, b.data(), b.data() + (m - n), m, c, K, n, m, &ds, &sc);
            const int want = restated(mx, a, b, c, K, &ds2, &sc2);
            CHECK(got == want);
            if (got && want) CHECK(ds == ds2 && sc == sc2);
            calls++;
            if (!got) continue;
            certified++;
            int64_t D = 0;
            for (int64_t i = 0; i < n; i++) D += mx.R[a[i]] - mx.w[a[i] * 5 + b[c + i]];
            if (D > -mx.o) second++;
        }
        int64_t cs = 0; // the scan as the host entry runs it: a read without a mismatch has a hit on diagonal c
        const int hit = gnx_cert_scan_naive(a.data(), n, b.data(), m, 16, &cs);
        if (nm == 0 && k % 32 != 9 && hit) CHECK(cs == c);
    }
    printf("cert_decide_test: %lld decisions, %lld certified, %lld of them with deficit > -o, %d failures\n", (long long)calls, (long long)certified, (long long)second, fails);
    CHECK(second >= 100);
    return fails ? 1 : 0;
}
