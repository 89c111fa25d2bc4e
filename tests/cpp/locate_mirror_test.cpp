// LocateBatch / AffineGapLocalEnd of include/gonomics_align.hpp from compiled C++: score and target end equal what the route of
// AffineGapLocal gives (its score; the target length minus its trailing ColD run).
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int64_t end_of(const std::vector<dna::Base> &target, const std::vector<align::Cigar> &route) {
    int64_t e = (int64_t)target.size();
    if (!route.empty() && route.back().Op == align::ColD) e -= route.back().RunLength;
    return e;
}

int main() {
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the locate entries refuse like the align entries
        try { align::AffineGapLocalEnd(dna::StringToBases("ACGTACGT"), dna::StringToBases("ACG"), align::DefaultScoreMatrix(), -400, -30); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(11);
    auto seq = [&](size_t n) { std::vector<dna::Base> v(n); for (auto &x : v) x = (dna::Base)(rng() % 4); return v; };
    std::vector<std::vector<dna::Base>> targets, queries;
    for (int k = 0; k < 40; k++) {
        targets.push_back(seq(1 + rng() % 900));
        const auto &t = targets.back();
        if (k % 2 == 0 && t.size() > 60) { const size_t o = rng() % (t.size() - 50); queries.emplace_back(t.begin() + (long)o, t.begin() + (long)o + 50); }
        else queries.push_back(seq(1 + rng() % 400));
    }
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    std::vector<int64_t> sc; std::vector<std::vector<align::Cigar>> rt;
    align::AlignBatch(GNX_AFFINE_GAP_LOCAL, mx, -600, -150, 10000, 10000, targets, queries, sc, rt);
    const auto got = align::LocateBatch(mx, -600, -150, targets, queries);
    gnx_timing tm;
    CHECK(gnx_get_timing(&tm) == GNX_OK);
    CHECK(tm.fast_path == 8);
    CHECK(got.first == sc);
    bool inside = false;
    for (size_t k = 0; k < targets.size(); k++) { CHECK(got.second[k] == end_of(targets[k], rt[k])); inside = inside || got.second[k] < (int64_t)targets[k].size(); }
    CHECK(inside);
    const auto one = align::AffineGapLocal(targets[0], queries[0], mx, -600, -150);
    const auto loc = align::AffineGapLocalEnd(targets[0], queries[0], mx, -600, -150);
    CHECK(loc.first == one.first && loc.second == end_of(targets[0], one.second));
    CHECK(align::LocateBatch(mx, -600, -150, {}, {}).first.empty());
    bool threw = false;
    try { align::AffineGapLocalEnd(targets[0], std::vector<dna::Base>{0, 9}, mx, -600, -150); } catch (const std::out_of_range &) { threw = true; }
    CHECK(threw);
    std::printf("locate mirror ok\n");
    return 0;
}
