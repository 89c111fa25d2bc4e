// The score-only functions of include/gonomics_align.hpp from compiled C++: every score equals the score of the align twin.
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the score entries refuse like the align entries
        try { align::AffineGapScore(dna::StringToBases("ACGT"), dna::StringToBases("ACG"), align::DefaultScoreMatrix(), -400, -30); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(7);
    auto seq = [&](size_t n) { std::vector<dna::Base> v(n); for (auto &x : v) x = (dna::Base)(rng() % 4); return v; };
    std::vector<std::vector<dna::Base>> alphas, betas;
    for (int k = 0; k < 40; k++) { alphas.push_back(seq(1 + rng() % 500)); betas.push_back(seq(1 + rng() % 500)); }
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    const int modes[] = {GNX_AFFINE_GAP, GNX_CONST_GAP, GNX_AFFINE_GAP_HIGHMEM, GNX_AFFINE_GAP_LOCAL, GNX_CONST_GAP_HIGHMEM};
    for (int mode : modes) {
        std::vector<int64_t> sc; std::vector<std::vector<align::Cigar>> rt;
        align::AlignBatch(mode, mx, -600, -150, 10000, 10000, alphas, betas, sc, rt);
        const std::vector<int64_t> got = align::ScoreBatch(mode, mx, -600, -150, alphas, betas);
        CHECK(got == sc);
        gnx_timing tm;
        CHECK(gnx_get_timing(&tm) == GNX_OK);
        CHECK((tm.fast_path == 7) == (mode != GNX_AFFINE_GAP_LOCAL));
    }
    const auto a = alphas[0], b = betas[0];
    CHECK(align::AffineGapScore(a, b, mx, -600, -150) == align::AffineGap(a, b, mx, -600, -150).first);
    CHECK(align::ConstGapScore(a, b, mx, -600) == align::ConstGap(a, b, mx, -600).first);
    CHECK(align::AffineGapLocalScore(a, b, mx, -600, -150) == align::AffineGapLocal(a, b, mx, -600, -150).first);
    CHECK(align::ScoreBatch(GNX_AFFINE_GAP, mx, -600, -150, {}, {}).empty());
    bool threw = false;
    try { align::AffineGapScore(std::vector<dna::Base>{0, 9}, b, mx, -600, -150); } catch (const std::out_of_range &) { threw = true; }
    CHECK(threw);
    std::printf("score mirror ok\n");
    return 0;
}
