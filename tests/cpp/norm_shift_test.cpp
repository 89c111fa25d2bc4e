// norm_shift_test.cpp -- csrc/norm_shift.h on the CPU: the chunk comparison, the key rotation and their composition into a shift, the way
// norm_shift_kernel composes them (a lane alone, and 64 lanes 32 bases apart with the first short run closing the total), against the
// rule's one-base-at-a-time loops.  The reference is packed here by hand into arrays of exactly the needed size, so that the address
// sanitizer this program is built with sees any read outside them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "norm_shift.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (g_fail++ < 20) fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

struct Packed {
    std::vector<uint8_t> codes;          // 0 .. 3, 4 = N
    std::vector<unsigned> b2;            // 16 bases a dword, the low base in the low bits
    std::vector<unsigned long long> bflag; // a bit per 64-base block that holds an N
    explicit Packed(const std::vector<uint8_t> &c) : codes(c) {
        const size_t n = c.size();
        b2.assign((n + 15) / 16, 0u);
        bflag.assign(((n + 63) / 64 + 63) / 64, 0ull);
        for (size_t k = 0; k < n; k++) {
            b2[k >> 4] |= (unsigned)(c[k] & 3) << (2 * (k & 15)); // (an N is packed as code 0: only the flag tells)
            if (c[k] >= 4) bflag[k >> 12] |= 1ull << ((k >> 6) & 63);
        }
    }
    int at(int64_t x) const {
        if (x < 0 || x >= (int64_t)codes.size()) { fprintf(stderr, "read outside the reference at %lld\n", (long long)x); abort(); }
        return codes[(size_t)x];
    }
};

// ---- the rule, literally ----
static int64_t loop_deletion(const Packed &R, int64_t x, int64_t L, int64_t lo) {
    while (x - 1 >= lo && R.codes[x - 1] < 4 && R.codes[x - 1] == R.codes[x + L - 1]) x--;
    return x;
}
static int64_t loop_insertion(const Packed &R, int64_t x, std::vector<int> &s, int64_t lo) {
    while (x - 1 >= lo && R.codes[x] < 4 && s.back() < 4 && R.codes[x] == s.back()) {
        s.insert(s.begin(), R.codes[x]);
        s.pop_back();
        x--;
    }
    return x;
}
static uint64_t pack(const std::vector<int> &s) {
    uint64_t v = 0;
    for (size_t k = 0; k < s.size(); k++) v |= (uint64_t)((s[k] < 4 ? s[k] : 4) + 1) << (3 * k);
    return v;
}

// ---- the kernel's composition ----
struct Shift { int64_t d; uint64_t key; };
// lane_chunks: chunks taken alone; coop: the rest by 64 simulated lanes (else alone to the end)
static Shift shift_of(const Packed &R, int kind, int64_t x, uint64_t key, int64_t lo, int lane_chunks, bool coop) {
    auto at = [&](int64_t p) { return R.at(p); };
    const int64_t xr = x - lo;
    int64_t L = 0, y = 0, rem = 0, d = 0;
    if (kind == 1) { L = (int64_t)key; y = x - 1; rem = xr; }
    else {
        L = norm_key_len(key);
        d = norm_ins_head(at, key, (int)L, x, xr);
        if (d == L) { y = x - L; rem = xr - L; }
    }
    bool open = rem > 0;
    for (int c = 0; (c < lane_chunks || !coop) && open; c++) {
        const int r = norm_chunk_run(R.b2.data(), R.bflag.data(), at, y, L, rem);
        d += r; y -= r; rem -= r;
        open = r == NORM_CHUNK && rem > 0;
    }
    while (open) { // one step of the wave
        int first = -1, rf = 0;
        for (int lane = 0; lane < 64 && first < 0; lane++) {
            const int64_t my = rem - (int64_t)NORM_CHUNK * lane;
            const int r = my > 0 ? norm_chunk_run(R.b2.data(), R.bflag.data(), at, y - (int64_t)NORM_CHUNK * lane, L, my) : 0;
            if (r < NORM_CHUNK) { first = lane; rf = r; }
        }
        if (first >= 0) { d += (int64_t)NORM_CHUNK * first + rf; open = false; }
        else { d += 64 * NORM_CHUNK; y -= 64 * NORM_CHUNK; rem -= 64 * NORM_CHUNK; }
    }
    Shift out;
    out.d = d;
    out.key = kind == 2 ? norm_key_rotate(key, (int)L, d) : key;
    return out;
}

static void check_deletion(const Packed &R, int64_t x, int64_t L, int64_t lo) {
    const int64_t want = loop_deletion(R, x, L, lo);
    for (int coop = 0; coop < 2; coop++) {
        const Shift s = shift_of(R, 1, x, (uint64_t)L, lo, 1, coop != 0);
        if (x - s.d != want) fprintf(stderr, "deletion (%lld, %lld) lo %lld coop %d: %lld, want %lld\n", (long long)x, (long long)L, (long long)lo, coop, (long long)(x - s.d), (long long)want);
        CHECK(x - s.d == want && s.key == (uint64_t)L);
    }
}
static void check_insertion(const Packed &R, int64_t x, const std::vector<int> &s0, int64_t lo) {
    std::vector<int> s = s0;
    const int64_t want = loop_insertion(R, x, s, lo);
    for (int coop = 0; coop < 2; coop++) {
        const Shift got = shift_of(R, 2, x, pack(s0), lo, 1, coop != 0);
        if (x - got.d != want || got.key != pack(s)) fprintf(stderr, "insertion of %d behind %lld lo %lld coop %d: %lld, want %lld\n", (int)s0.size(), (long long)x, (long long)lo, coop, (long long)(x - got.d), (long long)want);
        CHECK(x - got.d == want && got.key == pack(s));
    }
}

static std::vector<uint8_t> letters(const char *t) {
    std::vector<uint8_t> v;
    for (; *t; t++) v.push_back(*t == 'A' ? 0 : *t == 'C' ? 1 : *t == 'G' ? 2 : *t == 'T' ? 3 : 4);
    return v;
}
static std::vector<int> bases(const char *t) {
    std::vector<int> v;
    for (uint8_t c : letters(t)) v.push_back(c);
    return v;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (unsigned)(g_rng >> 32); }

// a random reference of n bases with a repeat of `period` planted so that a deletion of L = period at x shifts by exactly `shift`:
// the unit is repeated over [x - shift, x + L) and the base before it breaks the period
static Packed planted(int64_t n, int64_t x, int period, int64_t shift) {
    std::vector<uint8_t> c((size_t)n);
    for (auto &b : c) b = (uint8_t)(rnd() & 3);
    std::vector<uint8_t> unit((size_t)period);
    for (auto &b : unit) b = (uint8_t)(rnd() & 3);
    if (period > 1 && unit[0] == unit[1]) unit[1] = (uint8_t)((unit[0] + 1) & 3);
    for (int64_t k = x - shift; k < x + period; k++) c[(size_t)k] = unit[(size_t)((k - (x - shift)) % period)];
    if (x - shift - 1 >= 0) c[(size_t)(x - shift - 1)] = (uint8_t)((c[(size_t)(x - shift - 1 + period)] + 1) & 3);
    return Packed(c);
}

int main() {
    // ---- the chunk routine alone: every alignment of both chunks, against the per-base count ----
    {
        std::vector<uint8_t> c(400);
        for (auto &b : c) b = (uint8_t)(rnd() & 3);
        for (int k = 0; k < 150; k++) c[(size_t)(200 + k)] = c[(size_t)(200 + k % 3)];
        const Packed R(c);
        for (int64_t s = 0; s + 32 <= 400; s++) {
            const uint64_t v = norm_chunk(R.b2.data(), s);
            for (int k = 0; k < 32; k++) CHECK((int)(v >> (2 * k) & 3) == c[(size_t)(s + k)]);
        }
        for (int64_t y = 31; y < 360; y++)
            for (int64_t L = 1; L <= 39 && y + L < 400; L++) {
                int want = 0;
                while (want < 32 && c[(size_t)(y - want)] == c[(size_t)(y - want + L)]) want++;
                CHECK(norm_run32(norm_chunk(R.b2.data(), y - 31), norm_chunk(R.b2.data(), y + L - 31)) == want);
                auto at = [&](int64_t p) { return R.at(p); };
                CHECK(norm_chunk_run(R.b2.data(), R.bflag.data(), at, y, L, 32) == want);
                int64_t rem = 1 + (int64_t)(rnd() % 40); // the region's start cuts the run
                if (rem > y + 1) rem = y + 1;
                CHECK(norm_chunk_run(R.b2.data(), R.bflag.data(), at, y, L, rem) == (want < rem ? want : (int)rem));
            }
    }
    // ---- the rotation ----
    for (int L = 1; L <= 21; L++) {
        std::vector<int> s((size_t)L);
        for (auto &b : s) b = (int)(rnd() % 5);
        for (int64_t d : {(int64_t)0, (int64_t)1, (int64_t)L - 1, (int64_t)L, (int64_t)L + 1, (int64_t)5000, (int64_t)1 << 40}) {
            std::vector<int> t((size_t)L);
            for (int k = 0; k < L; k++) t[(size_t)k] = s[(size_t)((((k - d) % L) + L) % L)];
            CHECK(norm_key_rotate(pack(s), L, d) == pack(t));
            CHECK(norm_key_len(pack(s)) == L);
        }
    }
    // ---- the pins of the rule ----
    {
        const Packed g1(letters("GATTTTTC")), g2(letters("GCACACAT")), g3(letters("GATTNTTC")), g4(letters("TTTTTTTC"));
        struct { const Packed *R; int kind; int64_t x; const char *s; int64_t L, lo, want; const char *ws; } pins[] = {
            {&g1, 1, 6, "", 1, 0, 2, ""}, {&g1, 1, 5, "", 2, 0, 2, ""}, {&g1, 2, 6, "T", 0, 0, 1, "T"}, {&g1, 2, 6, "TT", 0, 0, 1, "TT"},
            {&g1, 2, 6, "GT", 0, 0, 5, "TG"}, {&g1, 2, 6, "NT", 0, 0, 5, "TN"}, {&g2, 1, 5, "", 2, 0, 1, ""}, {&g2, 2, 6, "CA", 0, 0, 0, "CA"},
            {&g2, 2, 6, "ACA", 0, 0, 3, "ACA"}, {&g2, 1, 5, "", 2, 3, 3, ""}, {&g2, 2, 6, "CA", 0, 3, 3, "AC"}, {&g3, 1, 6, "", 1, 0, 5, ""},
            {&g4, 1, 6, "", 1, 0, 0, ""}, {&g4, 2, 6, "T", 0, 0, 0, "T"},
        };
        for (const auto &p : pins)
            for (int coop = 0; coop < 2; coop++) {
                const Shift s = shift_of(*p.R, p.kind, p.x, p.kind == 1 ? (uint64_t)p.L : pack(bases(p.s)), p.lo, 1, coop != 0);
                CHECK(p.x - s.d == p.want);
                if (p.kind == 2) CHECK(s.key == pack(bases(p.ws)));
                if (p.kind == 1) check_deletion(*p.R, p.x, p.L, p.lo); else check_insertion(*p.R, p.x, bases(p.s), p.lo);
            }
    }
    // ---- planted shifts at every x mod 16 ----
    const int64_t shifts[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2079, 2080, 2081, 5003};
    const int periods[] = {1, 2, 3, 7, 15, 16, 17, 21, 33, 100};
    for (int64_t shift : shifts)
        for (int period : periods)
            for (int m = 0; m < 16; m++) {
                const int64_t x = 5200 + 16 * (int64_t)(rnd() % 4) + m, n = x + period + 40 + (int64_t)(rnd() % 16);
                const Packed R = planted(n, x, period, shift);
                CHECK(loop_deletion(R, x, period, 0) == x - shift); // (the condition on the input)
                check_deletion(R, x, period, 0);
                check_deletion(R, x, period, x - shift + (shift > 3 ? 3 : 0)); // clamped by the region
                if (period <= 21) {
                    // the unit behind x - 1 + period ... an insertion of one unit behind x + period - 1 shifts like the deletion plus one unit
                    std::vector<int> s;
                    for (int k = 0; k < period; k++) s.push_back(R.codes[(size_t)(x + k)]);
                    check_insertion(R, x + period - 1, s, 0);
                    check_insertion(R, x + period - 1, s, x - shift + 1);
                    // d < L, d == L, d > L by a foreign base inside the inserted unit / the whole unit / the repeat
                    if (period > 1) {
                        std::vector<int> t = s;
                        t[(size_t)(rnd() % (unsigned)period)] = 4; // a read N
                        check_insertion(R, x + period - 1, t, 0);
                        t = s;
                        t[0] = (t[0] + 1) & 3;
                        check_insertion(R, x + period - 1, t, 0);
                    }
                }
            }
    // ---- N: inside the repeat, at a 64-base block edge, in a flagged block next to clean ones ----
    for (int64_t npos : {(int64_t)5000, (int64_t)5055, (int64_t)5056, (int64_t)5119, (int64_t)5120, (int64_t)5121, (int64_t)3000})
        for (int period : {1, 3, 7, 33})
            for (int m = 0; m < 16; m++) {
                const int64_t x = 5200 + m;
                std::vector<uint8_t> c = planted(x + period + 50, x, period, 5003).codes;
                c[(size_t)npos] = 4;
                const Packed R(c);
                CHECK(loop_deletion(R, x, period, 0) == npos + 1 || (period > 1 && loop_deletion(R, x, period, 0) > npos));
                check_deletion(R, x, period, 0);
                if (period <= 21) {
                    std::vector<int> s;
                    for (int k = 0; k < period; k++) s.push_back(c[(size_t)(x + k)]);
                    check_insertion(R, x + period - 1, s, 0);
                }
            }
    // ---- a repeat that reaches position 0, and random repeat references ----
    for (int period : {1, 2, 7, 21})
        for (int64_t x : {(int64_t)40, (int64_t)2100, (int64_t)4099}) {
            std::vector<uint8_t> c((size_t)(x + period + 20));
            for (size_t k = 0; k < c.size(); k++) c[k] = (uint8_t)((k % (size_t)period) * 7 % 4);
            const Packed R(c);
            check_deletion(R, x, period, 0);
            std::vector<int> s;
            for (int k = 0; k < period; k++) s.push_back(c[(size_t)(x + 1 + k)]);
            check_insertion(R, x, s, 0);
        }
    for (int round = 0; round < 3000; round++) {
        const int64_t n = 80 + (int64_t)(rnd() % 300);
        std::vector<uint8_t> c((size_t)n);
        const int period = 1 + (int)(rnd() % 5);
        for (size_t k = 0; k < c.size(); k++) c[k] = (rnd() % 23 == 0) ? (uint8_t)(rnd() % 5) : (uint8_t)((k % (size_t)period) % 4);
        const Packed R(c);
        const int64_t L = 1 + (int64_t)(rnd() % 24), x = 1 + (int64_t)(rnd() % (unsigned)(n - L - 1)), lo = (int64_t)(rnd() % (unsigned)(x + 1));
        check_deletion(R, x, L, lo);
        std::vector<int> s((size_t)(1 + rnd() % 21));
        for (auto &b : s) b = rnd() % 9 == 0 ? (int)(rnd() % 5) : (int)((rnd() % (unsigned)period) % 4);
        check_insertion(R, x, s, lo);
    }
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("norm_shift_test ok\n");
    return 0;
}
