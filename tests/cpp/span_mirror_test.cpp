// LocateSpanBatch / AffineGapLocalSpan of include/gonomics_align.hpp from compiled C++: score, target start and target end equal what
// the route of AffineGapLocal gives (its score; its leading ColD run; the target length minus its trailing ColD run).
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int64_t start_of(const std::vector<align::Cigar> &route) {
    return route.size() > 1 && route.front().Op == align::ColD ? route.front().RunLength : 0;
}
static int64_t end_of(const std::vector<dna::Base> &target, const std::vector<align::Cigar> &route) {
    int64_t e = (int64_t)target.size();
    if (!route.empty() && route.back().Op == align::ColD) e -= route.back().RunLength;
    return e;
}

int main() {
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the span entries refuse like the align entries
        try { align::AffineGapLocalSpan(dna::StringToBases("ACGTACGT"), dna::StringToBases("ACG"), align::DefaultScoreMatrix(), -400, -30); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(12);
    auto seq = [&](size_t n) { std::vector<dna::Base> v(n); for (auto &x : v) x = (dna::Base)(rng() % 4); return v; };
    // one mutated read from the middle of a target: a substitution, a deleted base, an inserted base
    const std::vector<dna::Base> target = seq(2000);
    std::vector<dna::Base> read(target.begin() + 900, target.begin() + 1050);
    read[20] = (dna::Base)((read[20] + 1) % 4);
    read.erase(read.begin() + 70);
    read.insert(read.begin() + 110, (dna::Base)2);
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    const auto one = align::AffineGapLocal(target, read, mx, -600, -150);
    const align::Span sp = align::AffineGapLocalSpan(target, read, mx, -600, -150);
    gnx_timing tm;
    CHECK(gnx_get_timing(&tm) == GNX_OK);
    CHECK(tm.fast_path == 10);
    CHECK(sp.Score == one.first);
    CHECK(sp.TargetStart == start_of(one.second));
    CHECK(sp.TargetEnd == end_of(target, one.second));
    CHECK(0 < sp.TargetStart && sp.TargetStart < sp.TargetEnd && sp.TargetEnd < (int64_t)target.size());
    CHECK(align::LocateSpanBatch(mx, -600, -150, {}, {}).empty());
    std::printf("span mirror ok\n");
    return 0;
}
