// norm_shift.h -- the arithmetic of left-normalising an indel allele against the packed reference, plain C++: no HIP
// header needed.  Shared by norm_shift_kernel (pile_norm.hip.h) and by tests/cpp/norm_shift_test.cpp on the CPU.
//
// The shift of an allele of length L is a run of positions y, y - 1, ... with R[y] == R[y + L], both A C G T.  The packed reference holds
// 16 bases per dword, base k in bits 2 * (k & 15) of word k >> 4, so 32 bases are one 64-bit value cut out of two or three dwords, and the
// run of 32 comparisons is the leading zero count of an XOR.  The 2-bit codes know no N: a chunk that touches a flagged 64-base block
// (KParams::bflag) is compared base by base through the caller's accessor, which returns 4 or 5 there.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNX_NORM_HD __host__ __device__
#else
#define GNX_NORM_HD
#endif

constexpr int NORM_CHUNK = 32; // bases a comparison step takes

// the 32 bases s .. s + 31 (s >= 0), base s lowest.  Reads the dwords that hold them and no other.
GNX_NORM_HD inline uint64_t norm_chunk(const unsigned *b2, int64_t s) {
    const int64_t w = s >> 4;
    const int sh = 2 * (int)(s & 15);
    const uint64_t lo = (uint64_t)b2[w] | (uint64_t)b2[w + 1] << 32;
    if (sh == 0) return lo;
    return lo >> sh | (uint64_t)b2[w + 2] << (64 - sh);
}

// how many bases match counted from the TOP of two chunks: 0 .. 32
GNX_NORM_HD inline int norm_run32(uint64_t a, uint64_t b) {
    const uint64_t z = a ^ b, m = (z | z >> 1) & 0x5555555555555555ull;
    return m ? __builtin_clzll(m) >> 1 : NORM_CHUNK;
}

// does a base of [s, e] (e - s < 64) lie in a flagged block?  bflag: one bit per 64-base block
GNX_NORM_HD inline bool norm_flagged(const unsigned long long *bflag, int64_t s, int64_t e) {
    const int64_t b0 = s >> 6, b1 = e >> 6;
    return (((bflag[b0 >> 6] >> (b0 & 63)) | (bflag[b1 >> 6] >> (b1 & 63))) & 1ull) != 0;
}

// One step of the scan: the comparisons R[y - k] == R[y - k + L] for k = 0, 1, ... while they hold, at most min(rem, 32) of them
// (rem >= 1: the steps the region still admits -- y - rem + 1 is the lowest position read, and the caller keeps it at or above the region's
// start).  A whole chunk clear of flagged blocks is two 64-bit values; anything else goes base by base through at(x) (0 .. 3, or >= 4 for
// a base that matches nothing).
template <class At>
GNX_NORM_HD inline int norm_chunk_run(const unsigned *b2, const unsigned long long *bflag, At at, int64_t y, int64_t L, int64_t rem) {
    if (rem >= NORM_CHUNK && !norm_flagged(bflag, y - (NORM_CHUNK - 1), y) && !norm_flagged(bflag, y + L - (NORM_CHUNK - 1), y + L))
        return norm_run32(norm_chunk(b2, y - (NORM_CHUNK - 1)), norm_chunk(b2, y + L - (NORM_CHUNK - 1)));
    const int n = rem < NORM_CHUNK ? (int)rem : NORM_CHUNK;
    int k = 0;
    for (; k < n; k++) {
        const int c = at(y - k);
        if (c >= 4 || c != at(y - k + L)) break;
    }
    return k;
}

// the digits (3 bits each: code + 1, a read N = 5, the first base lowest) of a packed inserted sequence
GNX_NORM_HD inline int norm_key_len(uint64_t key) { return key ? (66 - __builtin_clzll(key)) / 3 : 0; }

// An insertion of L bases shifted left by d becomes s'[k] = s[(k - d) mod L]: the bases the shift passed were equal to the sequence's own,
// one period after the other, so the new sequence is a rotation of the old one and needs no reference read.
GNX_NORM_HD inline uint64_t norm_key_rotate(uint64_t key, int L, int64_t d) {
    const int r = L > 0 ? (int)(d % L) : 0;
    if (r == 0) return key;
    const uint64_t mask = ((uint64_t)1 << (3 * L)) - 1ull; // (L <= 21: 63 bits)
    return (key << (3 * r) | key >> (3 * (L - r))) & mask;
}

// The comparisons of an insertion that are against its own bases: R[x - k] == s[L - 1 - k] for k = 0 .. min(L, rem) - 1 while they hold.
// A digit 5 (a read N) matches nothing, and neither does a reference base >= 4.
template <class At>
GNX_NORM_HD inline int norm_ins_head(At at, uint64_t key, int L, int64_t x, int64_t rem) {
    const int n = rem < L ? (int)rem : L;
    int k = 0;
    for (; k < n; k++) {
        const int c = at(x - k);
        if (c >= 4 || (int)(key >> (3 * (L - 1 - k)) & 7ull) != c + 1) break;
    }
    return k;
}
