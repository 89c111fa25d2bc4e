// fp_rounds_test.cpp -- gonomics_amd/csrc/fp_rounds.h alone in a host program (built with the address and undefined-behaviour sanitizers
// by tests/test_fp_rounds_cpp.py): for every pair count from 0 to past four rounds of 1, 2 and 256 CUs and with rounds of 1, 2, 3, 768 and
// 3 x n_cu workgroups, the launches cover [0, cnt) once and in order, none is empty, the first of two is a whole number of rounds, a launch
// that is alone is whole rounds or less than one round, and every grid is what its count needs.  The form rule: the four-wave form on
// one interval of pair counts that scales with the CUs, the one-wave form below and above it.
#include <cstdio>
#include <cstdint>
#include "../../gonomics_amd/csrc/fp_rounds.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static long long check_plan(int64_t cnt, int64_t round_wgs, int wg_pairs) {
    GnxFpLaunch ln[2] = {{-1, -1, -1}, {-1, -1, -1}};
    const int nl = gnx_fp_round_plan(cnt, round_wgs, wg_pairs, ln);
    CHECK(nl >= 0 && nl <= 2, "cnt %lld round %lld: %d launches", (long long)cnt, (long long)round_wgs, nl);
    CHECK((nl == 0) == (cnt <= 0), "cnt %lld round %lld: %d launches", (long long)cnt, (long long)round_wgs, nl);
    int64_t at = 0;
    for (int x = 0; x < nl; x++) {
        CHECK(ln[x].first == at, "cnt %lld round %lld launch %d: first %lld, expected %lld", (long long)cnt, (long long)round_wgs, x, (long long)ln[x].first, (long long)at);
        CHECK(ln[x].count > 0, "cnt %lld round %lld launch %d: empty", (long long)cnt, (long long)round_wgs, x);
        CHECK(ln[x].grid == (ln[x].count + wg_pairs - 1) / wg_pairs, "cnt %lld round %lld launch %d: grid %lld for %lld pairs", (long long)cnt, (long long)round_wgs, x, (long long)ln[x].grid, (long long)ln[x].count);
        at += ln[x].count;
    }
    CHECK(at == (cnt > 0 ? cnt : 0), "cnt %lld round %lld: %lld pairs covered", (long long)cnt, (long long)round_wgs, (long long)at);
    if (round_wgs <= 0) { CHECK(nl <= 1, "cnt %lld: split without a round size", (long long)cnt); return nl; }
    if (nl == 2) { // whole rounds of full workgroups, then less than one round
        CHECK(ln[0].grid % round_wgs == 0 && ln[0].count == ln[0].grid * wg_pairs, "cnt %lld round %lld: first launch %lld workgroups, %lld pairs", (long long)cnt, (long long)round_wgs, (long long)ln[0].grid, (long long)ln[0].count);
        CHECK(ln[1].grid < round_wgs, "cnt %lld round %lld: remainder of %lld workgroups", (long long)cnt, (long long)round_wgs, (long long)ln[1].grid);
    } else if (nl == 1) {
        CHECK(ln[0].grid % round_wgs == 0 || ln[0].grid < round_wgs, "cnt %lld round %lld: single launch of %lld workgroups", (long long)cnt, (long long)round_wgs, (long long)ln[0].grid);
    }
    return nl;
}

int main() {
    long long plans = 0, split = 0;
    const int n_cus[3] = {1, 2, 256};
    for (int c = 0; c < 3; c++) {
        const int n_cu = n_cus[c];
        const int64_t rounds[5] = {1, 2, 3, 768, (int64_t)GNX_FP_WG4_PER_CU * n_cu};
        const int64_t top = (int64_t)4 * 32 * (3 * n_cu) + 40;
        for (int o = 0; o < 5; o++)
            for (int64_t cnt = 0; cnt <= top; cnt++) { split += check_plan(cnt, rounds[o], 32) == 2; plans++; }
        for (int64_t cnt = 0; cnt <= top; cnt += 7) { check_plan(cnt, 0, 32); plans++; } // no round size: one launch
        // the form rule: one interval [lo, hi] of the four-wave form, lo = three workgroups per CU
        int64_t lo = -1, hi = -1, changes = 0;
        int prev = GNX_FP_FORM_WAVE;
        for (int64_t cnt = 0; cnt <= (int64_t)1000 * n_cu; cnt++) {
            const int f = gnx_fp_sweep_form(cnt, n_cu);
            CHECK(f == GNX_FP_FORM_WAVE || f == GNX_FP_FORM_WG4, "form %d for %lld pairs on %d CUs", f, (long long)cnt, n_cu);
            if (f != prev) { changes++; if (f == GNX_FP_FORM_WG4) lo = cnt; else hi = cnt - 1; }
            prev = f;
        }
        CHECK(changes == 2 && lo == (int64_t)96 * n_cu && hi == (int64_t)100000 * n_cu / 256, "n_cu %d: four-wave form on [%lld, %lld], %lld changes", n_cu, (long long)lo, (long long)hi, (long long)changes);
    }
    CHECK(gnx_fp_sweep_form(35820, 256) == GNX_FP_FORM_WG4 && gnx_fp_sweep_form(24575, 256) == GNX_FP_FORM_WAVE && gnx_fp_sweep_form(24576, 256) == GNX_FP_FORM_WG4 &&
          gnx_fp_sweep_form(100000, 256) == GNX_FP_FORM_WG4 && gnx_fp_sweep_form(100001, 256) == GNX_FP_FORM_WAVE && gnx_fp_sweep_form(64, 256) == GNX_FP_FORM_WAVE, "the rule on 256 CUs");
    check_plan(-5, 3, 32);
    // the cases the device test splits: rounds of one and two workgroups around exact multiples
    {
        GnxFpLaunch ln[2];
        CHECK(gnx_fp_round_plan(64, 2, 32, ln) == 1 && ln[0].count == 64 && ln[0].grid == 2, "64 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(65, 2, 32, ln) == 2 && ln[0].count == 64 && ln[1].first == 64 && ln[1].count == 1 && ln[1].grid == 1, "65 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(63, 2, 32, ln) == 1 && ln[0].count == 63 && ln[0].grid == 2, "63 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(33, 2, 32, ln) == 1 && ln[0].count == 33 && ln[0].grid == 2, "33 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(33, 1, 32, ln) == 1 && ln[0].count == 33 && ln[0].grid == 2, "33 pairs, rounds of 1: two rounds, the second short of pairs");
        CHECK(gnx_fp_round_plan(96, 2, 32, ln) == 2 && ln[0].count == 64 && ln[1].first == 64 && ln[1].count == 32 && ln[1].grid == 1, "96 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(97, 3, 32, ln) == 2 && ln[0].count == 96 && ln[1].count == 1, "97 pairs, rounds of 3");
        CHECK(gnx_fp_round_plan(97, 2, 32, ln) == 1 && ln[0].count == 97 && ln[0].grid == 4, "97 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(129, 2, 32, ln) == 2 && ln[0].count == 128 && ln[1].count == 1, "129 pairs, rounds of 2");
        CHECK(gnx_fp_round_plan(35820, 768, 32, ln) == 2 && ln[0].count == 24576 && ln[0].grid == 768 && ln[1].count == 11244 && ln[1].grid == 352, "the headline's live pairs");
    }
    printf("fp_rounds_test: %lld plans, %lld of them two launches, %d failures\n", plans, split, fails);
    return fails ? 1 : 0;
}
