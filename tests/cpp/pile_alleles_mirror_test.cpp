// PileupTrackAlleles / PileupAlleles / PileupIndelCalls of include/gonomics_align.hpp from compiled C++: the worked values of gnx_align.h
// and one pile with two alleles at one position.
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    static_assert(sizeof(gnx_pile_allele) == 32 && sizeof(gnx_pile_indel_call) == 40, "the layouts of gnx_align.h");
    // no pile: every entry refuses
    CHECK(gnx_pileup_close() == GNX_OK);
    gnx_pile_allele *al = nullptr;
    int64_t n = -1;
    CHECK(gnx_pileup_track_alleles(0) == GNX_EINVAL && gnx_pileup_allele_info(nullptr, nullptr, nullptr) == GNX_EINVAL && gnx_pileup_alleles(&al, &n) == GNX_EINVAL);
    CHECK(al == nullptr && n == -1);
    if (gnx_device_count() <= 0) {
        try { align::PileupOpen(0, 10); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(43);
    Seq genome(400);
    for (auto &x : genome) x = (dna::Base)(rng() % 4);
    const Seq a0 = dna::StringToBases("ACGTACGTAC");
    std::copy(a0.begin(), a0.end(), genome.begin() + 100);
    if (gnx_set_reference(genome.data(), (int64_t)genome.size())) return 1;
    const std::vector<align::Cigar> r0 = {{6, align::ColM}, {1, align::ColD}, {3, align::ColM}}, r1 = {{4, align::ColM}, {2, align::ColI}, {6, align::ColM}},
                                    r2 = {{3, align::ColD}, {2, align::ColI}, {4, align::ColM}, {3, align::ColD}}, r3 = {{4, align::ColM}, {1, align::ColI}, {6, align::ColM}};
    // a pile that does not track has no alleles to give
    align::PileupOpen(0, 400);
    CHECK(gnx_pileup_alleles(&al, &n) == GNX_EINVAL);
    align::PileupTrackAlleles();
    CHECK(align::PileupAlleles().empty());
    // the three worked values (strands 0, 1, 0), and a second, shorter insertion behind 103 on strand 1
    align::PileupAdd(mx, -600, -150, {dna::StringToBases("ACGAACTAC"), dna::StringToBases("ACGTTTACGTAC"), dna::StringToBases("TTTACG"), dna::StringToBases("ACGTGACGTAC"), dna::StringToBases("ACGTTTACGTAC")},
                     {{100, 10}, {100, 10}, {100, 10}, {100, 10}, {100, 10}}, {0, 1, 0, 1, 0}, {r0, r1, r2, r3, r1});
    const auto alleles = align::PileupAlleles();
    CHECK(alleles.size() == 3);
    CHECK(alleles[0].pos == 103 && alleles[0].kind == 2 && alleles[0].length == 1 && alleles[0].seq == 3 && alleles[0].count == 1 && alleles[0].count_fwd == 0);
    CHECK(alleles[1].pos == 103 && alleles[1].kind == 2 && alleles[1].length == 2 && alleles[1].seq == 36 && alleles[1].count == 2 && alleles[1].count_fwd == 1);
    CHECK(alleles[2].pos == 106 && alleles[2].kind == 1 && alleles[2].length == 1 && alleles[2].seq == 0 && alleles[2].count == 1 && alleles[2].count_fwd == 1);
    CHECK(align::PileupAlleleBases(36) == dna::StringToBases("TT"));
    int32_t tracking = 0;
    int64_t events = 0, bytes = 0;
    CHECK(gnx_pileup_allele_info(&tracking, &events, &bytes) == GNX_OK && tracking == 1 && events == 4 && bytes > 0);
    CHECK(align::PileupInfo().DeviceBytes == 400 * 56);
    // depth is 5 at 103 and at 106 (the third read's M columns lie over both): nothing reaches a half, a third only the two-read insertion
    CHECK(align::PileupIndelCalls().empty());
    align::PileCallOpts o;
    o.FracDen = 3;
    const auto calls = align::PileupIndelCalls(o);
    CHECK(calls.size() == 1 && calls[0].pos == 103 && calls[0].seq == 36 && calls[0].depth == 5 && calls[0].count == 2 && calls[0].count_fwd == 1 && calls[0].ref == genome[103]);
    o.FracDen = 5;
    CHECK(align::PileupIndelCalls(o).size() == 3);
    // tracking is refused once reads are in, and goes with the pile
    CHECK(gnx_pileup_track_alleles(0) == GNX_EINVAL);
    align::PileupOpen(0, 400);
    CHECK(gnx_pileup_allele_info(&tracking, &events, &bytes) == GNX_OK && tracking == 0 && events == 0 && bytes == 0);
    gnx_set_reference(nullptr, 0);
    CHECK(gnx_pileup_allele_info(nullptr, nullptr, nullptr) == GNX_EINVAL);
    std::printf("pile alleles mirror ok%s\n", "");
    return 0;
}
