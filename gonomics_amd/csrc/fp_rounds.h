// fp_rounds.h -- which form of the one-block sweep a batch gets, and how the four-wave form (fp_sweep_kernel<.., 4>, DESIGN.md section
// 4.1) is cut into launches: plain C++, no HIP header needed (tests/cpp/fp_rounds_test.cpp runs it on the host).
// A ROUND is what the device holds at once: round_wgs workgroups (3 per CU by LDS) of wg_pairs pairs (4 waves x 8).  The split form
// launches the largest whole number of rounds -- every CU holds three workgroups, (3,3,3,3) waves on its SIMDs, and a workgroup that
// ends is replaced on its own CU, the only one with a free slot -- and then the remainder onto an empty device.  Measured
// (profiles/sweep_rounds.json), it is never faster than the same workgroups in ONE launch and 0.5 - 0.7 ms slower wherever the two
// differ: the drain between the launches costs more than the even start buys.  It stays behind GNX_FP_ROUND (tests, measurements).
#pragma once
#include <stdint.h>

enum { GNX_FP_WG4_PER_CU = 3 }; // four-wave workgroups a CU holds: 42 of its 128 LDS granules each

// The forms of the one-block sweep: one-wave workgroups, or four-wave workgroups (one wave on each SIMD of the CU).
enum { GNX_FP_FORM_WAVE = 0, GNX_FP_FORM_WG4 = 1 };

// Which form sweeps cnt pairs on n_cu CUs: the four-wave form from three workgroups per CU on (24 576 pairs on 256 CUs) up to the
// largest batch measured (100 000 pairs on 256 CUs), the one-wave form below and above.  profiles/sweep_rounds.json: from 24 576 to
// 81 920 pairs the four-wave form takes 1.6 - 1.8 ms less wherever the one-wave form's 11 slots per CU leave a twelfth wave over and the
// same time elsewhere; at 8 192 - 20 480 pairs, where no SIMD holds more than two waves either way, and at 100 000 they take the same time.
inline int gnx_fp_sweep_form(int64_t cnt, int n_cu) {
    const int64_t cus = n_cu > 0 ? n_cu : 1;
    const int64_t lo = (int64_t)GNX_FP_WG4_PER_CU * 32 * cus, hi = (int64_t)100000 * cus / 256;
    return (cnt >= lo && cnt <= hi) ? GNX_FP_FORM_WG4 : GNX_FP_FORM_WAVE;
}

struct GnxFpLaunch {
    int64_t first; // first pair of the launch
    int64_t count; // its pairs: [first, first + count)
    int64_t grid;  // its workgroups: ceil(count / wg_pairs)
};

// The launches of cnt pairs, in order: out[0 .. returned), at most two.  Every pair falls in exactly one launch and no launch is empty
// (cnt <= 0: none).  When there are two, the first holds a whole number of rounds of full workgroups; a single launch is either whole
// rounds (its last workgroup may be short of pairs) or less than one round.  round_wgs <= 0: one launch, never split.
inline int gnx_fp_round_plan(int64_t cnt, int64_t round_wgs, int wg_pairs, GnxFpLaunch out[2]) {
    if (cnt <= 0 || wg_pairs <= 0) return 0;
    const int64_t wgs = (cnt + wg_pairs - 1) / wg_pairs;
    const int64_t main_wgs = round_wgs > 0 ? wgs / round_wgs * round_wgs : wgs;
    const int64_t main_cnt = main_wgs * wg_pairs < cnt ? main_wgs * wg_pairs : cnt;
    int k = 0;
    if (main_cnt > 0) { out[k].first = 0; out[k].count = main_cnt; out[k].grid = main_wgs; k++; }
    if (cnt > main_cnt) { out[k].first = main_cnt; out[k].count = cnt - main_cnt; out[k].grid = wgs - main_wgs; k++; }
    return k;
}
