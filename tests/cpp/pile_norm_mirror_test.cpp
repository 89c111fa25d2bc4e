// PileupAlleles(normalize) / PileupIndelCalls(opts, normalize) of include/gonomics_align.hpp from compiled C++: one deletion placed at three
// bases of a homopolymer is three alleles for the plain query and one, at the leftmost base, for the normalised one.
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    // no pile: both entries refuse and write nothing
    CHECK(gnx_pileup_close() == GNX_OK);
    gnx_pile_allele *al = nullptr;
    gnx_pile_indel_call *ic = nullptr;
    int64_t n = -1;
    const gnx_pile_call_opts co = {1, 1, 1, 2, 0, 0};
    CHECK(gnx_pileup_alleles_norm(&al, &n) == GNX_EINVAL && gnx_pileup_indel_calls_norm(&co, &ic, &n) == GNX_EINVAL);
    CHECK(gnx_pileup_alleles_norm(nullptr, &n) == GNX_EINVAL && gnx_pileup_indel_calls_norm(nullptr, &ic, &n) == GNX_EINVAL);
    CHECK(al == nullptr && ic == nullptr && n == -1);
    if (gnx_device_count() <= 0) {
        try { align::PileupOpen(0, 10); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(47);
    Seq genome(400);
    for (auto &x : genome) x = (dna::Base)(rng() % 4);
    const Seq a0 = dna::StringToBases("GATTTTTC");
    std::copy(a0.begin(), a0.end(), genome.begin() + 100);
    if (gnx_set_reference(genome.data(), (int64_t)genome.size())) return 1;
    const std::vector<align::Cigar> d2 = {{2, align::ColM}, {1, align::ColD}, {5, align::ColM}}, d4 = {{4, align::ColM}, {1, align::ColD}, {3, align::ColM}},
                                    d6 = {{6, align::ColM}, {1, align::ColD}, {1, align::ColM}}, i6 = {{7, align::ColM}, {1, align::ColI}, {1, align::ColM}};
    // a pile that does not track has no alleles to give
    align::PileupOpen(0, 400);
    CHECK(gnx_pileup_alleles_norm(&al, &n) == GNX_EINVAL && gnx_pileup_indel_calls_norm(&co, &ic, &n) == GNX_EINVAL);
    align::PileupTrackAlleles();
    CHECK(align::PileupAlleles(true).empty() && align::PileupIndelCalls(align::PileCallOpts(), true).empty());
    align::PileupAdd(mx, -600, -150, {dna::StringToBases("GATTTTC"), dna::StringToBases("GATTTTC"), dna::StringToBases("GATTTTC"), dna::StringToBases("GATTTTTTC")},
                     {{100, 8}, {100, 8}, {100, 8}, {100, 8}}, {0, 1, 0, 1}, {d2, d4, d6, i6});
    const auto plain = align::PileupAlleles();
    CHECK(plain.size() == 4 && plain[0].pos == 102 && plain[1].pos == 104 && plain[2].pos == 106 && plain[2].kind == 1 && plain[3].pos == 106 && plain[3].kind == 2);
    const auto norm = align::PileupAlleles(true);
    CHECK(norm.size() == 2);
    CHECK(norm[0].pos == 101 && norm[0].kind == 2 && norm[0].length == 1 && norm[0].seq == 4 && norm[0].count == 1 && norm[0].count_fwd == 0);
    CHECK(norm[1].pos == 102 && norm[1].kind == 1 && norm[1].length == 1 && norm[1].seq == 0 && norm[1].count == 3 && norm[1].count_fwd == 2);
    // the log stays raw
    const auto again = align::PileupAlleles();
    CHECK(again.size() == 4 && again[1].pos == 104 && again[1].count == 1);
    // depth is 4 everywhere: no plain allele reaches a half, the merged deletion does
    CHECK(align::PileupIndelCalls().empty());
    const auto calls = align::PileupIndelCalls(align::PileCallOpts(), true);
    CHECK(calls.size() == 1 && calls[0].pos == 102 && calls[0].kind == 1 && calls[0].length == 1 && calls[0].count == 3 && calls[0].count_fwd == 2 && calls[0].depth == 4 && calls[0].ref == 3);
    gnx_timing t;
    CHECK(gnx_get_timing(&t) == GNX_OK && t.fast_path == 19);
    gnx_set_reference(nullptr, 0);
    std::printf("pile norm mirror ok%s\n", "");
    return 0;
}
