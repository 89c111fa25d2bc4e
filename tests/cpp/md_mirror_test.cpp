// MDTags / MDTagsByOffset / Mapq of include/gonomics_align.hpp from compiled C++: the MD strings of the routes AlignBatch returns are
// checked against a column-by-column restatement written here; the resident reference gives what the same bytes give.
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

// the walk of gnx_align.h on the expanded columns
static std::string restate(int mode, const Seq &a, const Seq &b, const std::vector<align::Cigar> &route) {
    std::vector<int> cols;
    for (const auto &c : route) for (int64_t k = 0; k < c.RunLength; k++) cols.push_back(c.Op);
    size_t lo = 0, hi = cols.size();
    if (mode == GNX_AFFINE_GAP_LOCAL) {
        while (lo < cols.size() && cols[lo] == align::ColD) lo++;
        while (hi > lo && cols[hi - 1] == align::ColD) hi--;
    }
    std::string md;
    size_t i = 0, j = 0;
    int64_t run = 0;
    for (size_t k = 0; k < cols.size(); k++) {
        const bool inside = k >= lo && k < hi;
        if (cols[k] == align::ColM) {
            if (inside && a[i] == b[j]) run++;
            else if (inside) { md += std::to_string(run) + "ACGTN"[a[i]]; run = 0; }
            i++; j++;
        } else if (cols[k] == align::ColI) j++;
        else {
            const bool behind_d = k > lo && cols[k - 1] == align::ColD;
            if (inside && !behind_d) { md += std::to_string(run) + "^" + "ACGTN"[a[i]]; run = 0; }
            else if (inside) md += "ACGTN"[a[i]];
            i++;
        }
    }
    (void)j;
    return md + std::to_string(run);
}

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    // the MAPQ rule is host arithmetic: it needs no device
    const std::vector<int64_t> S = {0, -5, 400, 400, 400, 400, 400, 400, 400, 61, (int64_t)1 << 62}, S2 = {INT64_MIN, 3, INT64_MIN, -40, 400, 500, 399, 200, 1, 1, (int64_t)1 << 61};
    CHECK(align::Mapq(S, S2) == (std::vector<int>{0, 0, 60, 60, 0, 0, 0, 30, 59, 59, 30}) && align::Mapq({}, {}).empty());
    const Seq a0 = dna::StringToBases("ACGTACGTAC"), b0 = dna::StringToBases("ACGAACTAC"), b1 = dna::StringToBases("TTTACG");
    const std::vector<align::Cigar> r0 = {{6, align::ColM}, {1, align::ColD}, {3, align::ColM}}, r1 = {{3, align::ColD}, {2, align::ColI}, {4, align::ColM}, {3, align::ColD}};
    CHECK(restate(GNX_AFFINE_GAP_HIGHMEM, a0, b0, r0) == "3T2^G3" && restate(GNX_AFFINE_GAP_LOCAL, a0, b1, r1) == "4" && restate(GNX_AFFINE_GAP, a0, b1, r1) == "0^ACG4^TAC0");
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the call refuses like the align entries
        try { align::MDTags(GNX_AFFINE_GAP_HIGHMEM, mx, -600, -150, {a0}, {b0}, {r0}); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    CHECK(align::MDTags(GNX_AFFINE_GAP_HIGHMEM, mx, -600, -150, {a0}, {b0}, {r0}) == std::vector<std::string>{"3T2^G3"});
    CHECK(align::MDTags(GNX_AFFINE_GAP_LOCAL, mx, -600, -150, {a0, a0}, {b1, b0}, {r1, r0}) == (std::vector<std::string>{"4", "3T2^G3"}));
    CHECK(align::MDTags(GNX_AFFINE_GAP, mx, -600, -150, {a0}, {b1}, {r1}) == std::vector<std::string>{"0^ACG4^TAC0"});
    CHECK(align::MDTags(GNX_AFFINE_GAP, mx, -600, -150, {}, {}, {}).empty());
    std::mt19937 rng(32);
    auto seq = [&](size_t n) { Seq v(n); for (auto &x : v) x = (dna::Base)(rng() % 4); return v; };
    const Seq genome = seq(3000);
    for (int mode : {GNX_AFFINE_GAP_HIGHMEM, GNX_AFFINE_GAP_LOCAL, GNX_CONST_GAP_HIGHMEM}) {
        const bool local = mode == GNX_AFFINE_GAP_LOCAL;
        const int64_t go = mode == GNX_CONST_GAP_HIGHMEM ? -430 : -600, ge = mode == GNX_CONST_GAP_HIGHMEM ? 0 : -150;
        std::vector<Seq> reads, wins;
        std::vector<std::pair<int64_t, int64_t>> windows;
        for (int k = 0; k < 24; k++) {
            const int64_t at = (int64_t)(rng() % 2700), len = 100 + (int64_t)(rng() % 120);
            Seq rd(genome.begin() + at + 10, genome.begin() + at + 10 + 80 + (local ? 0 : len - 100));
            for (int e = 0; e < 4; e++) rd[rng() % rd.size()] = (dna::Base)(rng() % 4);
            rd.erase(rd.begin() + 40, rd.begin() + 40 + (k % 3));
            if (k % 4 == 3) rd.insert(rd.begin() + 20, (dna::Base)(rng() % 4));
            reads.push_back(rd);
            wins.push_back(Seq(genome.begin() + at, genome.begin() + at + len));
            windows.push_back({at, len});
        }
        // the window is the described side: alpha
        std::vector<int64_t> sc; std::vector<std::vector<align::Cigar>> rt;
        align::AlignBatch(mode, mx, go, ge, 10000, 10000, wins, reads, sc, rt);
        const auto got = align::MDTags(mode, mx, go, ge, wins, reads, rt);
        CHECK(got.size() == reads.size());
        size_t events = 0;
        for (size_t k = 0; k < got.size(); k++) { CHECK(got[k] == restate(mode, wins[k], reads[k], rt[k])); events += got[k].find('^') != std::string::npos; }
        CHECK(events > 0);
        if (!local) continue;
        // the same windows from the resident reference
        if (gnx_set_reference(genome.data(), (int64_t)genome.size())) return 1;
        const auto res = align::MDTagsByOffset(mx, go, ge, reads, windows, rt);
        gnx_set_reference(nullptr, 0);
        CHECK(res == got);
    }
    std::printf("md mirror ok%s\n", "");
    return 0;
}
