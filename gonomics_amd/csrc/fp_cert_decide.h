// fp_cert_decide.h -- the gapless-read certificate's decision arithmetic, plain C++: no HIP header needed.
// Shared by fp_cert_kernel (fp_cert.hip.h, one lane per pair runs it on staged bases) and by the host-only debug entry
// gnx_debug_gapless_certificate (the CPU tests).  Everything here is exact integer arithmetic in int64.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNX_CERT_HD __host__ __device__
#else
#define GNX_CERT_HD
#endif

// Per call, from gnx_params: w(x, y) = s(x, y) - 2e (the rebasing of section 4), R_x = w(x, x), lambda = the least loss of a read row
// that is mismatched or skipped.  ok = 0: the matrix (or gapOpen >= 0) admits no certificate.
struct GnxCertMatrix {
    int64_t w[25];
    int64_t R[4];
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
    mx->lambda = lam;
    mx->ok = (ok && lam > 0) ? 1 : 0;
}

// Items 1 (shape and checkerboard), 2 (no N in the read), 4, 5 and 6 of the certificate for a pair whose exact K-mer matches all lie on
// diagonal c (item 3, the caller's scan).  a[0..n) = the read; bd / bf / bl[0..n) = the window's bases under the read on diagonal c, on
// the window's first n columns and on its last n columns (b + c, b, b + m - n).  Item 4 has two branches: deficit < -o, or
// -o < deficit < -2o with the edge rule (a second pass over at most T2 rows from each end, running sums only).  Returns 1 and the
// closed form -- d* = the trailing read bases that sit on the window's last columns, the score -- or 0: the pair goes through the sweep.
GNX_CERT_HD inline int gnx_cert_decide(const GnxCertMatrix *mx, const uint8_t *a, int64_t n, const uint8_t *bd, const uint8_t *bf, const uint8_t *bl,
                                       int64_t m, int64_t c, int64_t K, int64_t ci, int64_t cj, int64_t *d_star, int64_t *score) {
    if (!mx->ok || n < 1 || K < 1 || m < n + 2 || c <= 0 || c >= m - n) return 0;
    if (ci < n || cj < m) return 0; // a checkerboard edge inside the matrix: quirks Q1 / Q2 are the walk's business
    int64_t deficit = 0, mid_sum = 0, F = 0;
    for (int64_t i = 0; i < n; i++) {
        const int x = a[i];
        if (x >= 4 || bd[i] >= 5 || bf[i] >= 5 || bl[i] >= 5) return 0;
        const int64_t mid = mx->w[x * 5 + bd[i]];
        deficit += mx->R[x] - mid;
        mid_sum += mid;
        F += mx->w[x * 5 + bf[i]] - mid; // the first i + 1 rows on the window's first columns instead (ties stay on the diagonal)
        if (F > 0) return 0;
    }
    const int64_t O = -mx->o;
    if (deficit == O || deficit >= 2 * O) return 0; // (deficit == -o: a perfect path with three gap runs ties; refused, not argued)
    const int64_t J = deficit / mx->lambda, J1 = (deficit + O) / mx->lambda;
    if (n - J <= 0 || n - J1 <= 0) return 0;
    if (K > (n - J + (3 + J) - 1) / (3 + J) || K > (n - J1 + (2 + J1) - 1) / (2 + J1)) return 0;
    if (deficit > O) {
        // -o < deficit < -2o: paths with three gap runs.  Off diagonal c they need an exact run of K rows (the third inequality); with a
        // segment on diagonal c they have to save -o or more on the rows outside it: at most T1 rows at one end and T2 at the other.
        const int64_t J3 = (deficit - O) / mx->lambda;
        if (K > (n - J3 + (4 + J3) - 1) / (4 + J3)) return 0;
        const int64_t T1 = (1 + J3) * (K - 1) + J3, T2 = (2 + J3) * (K - 1) + J3;
        if (T1 + T2 >= n) return 0; // (every row is an edge row: E = deficit)
        int64_t h1 = 0, h2 = 0, t1 = 0, t2 = 0; // the loss of the first / last T1 and T2 rows
        for (int64_t i = 0; i < T2; i++) {
            const int64_t lh = mx->R[a[i]] - mx->w[a[i] * 5 + bd[i]], lt = mx->R[a[n - 1 - i]] - mx->w[a[n - 1 - i] * 5 + bd[n - 1 - i]];
            h2 += lh; t2 += lt;
            if (i < T1) { h1 += lh; t1 += lt; }
        }
        if (h1 + t2 >= O || h2 + t1 >= O) return 0;
    }
    int64_t G = 0, best = 0, ds = 0;
    for (int64_t d = 1; d <= n; d++) { // the last d rows on the window's last columns instead: the LARGEST d that attains the maximum
        const int64_t i = n - d;
        G += mx->w[a[i] * 5 + bl[i]] - mx->w[a[i] * 5 + bd[i]];
        if (G >= best) { best = G; ds = d; }
    }
    if (ds >= n) return 0;
    *d_star = ds;
    *score = mid_sum + best + 2 * mx->o + mx->e * (n + m);
    return 1;
}

// Item 3 the naive way (host: the debug entry).  Exact K-mer matches of read positions q .. q + K - 1 and window positions j .. j + K - 1 over
// all q, j; window bytes that are not A C G T count as their two low bits, like in the kernel's rolling code (a false hit can only
// refuse).  Returns 1 and the diagonal when the matches are non-empty and share one diagonal c = j - q.
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
