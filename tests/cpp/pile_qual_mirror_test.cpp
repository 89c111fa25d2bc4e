// PileupTrackQualities / PileupAdd with qualities / PileupGetQual / PileupGenotypes of include/gonomics_align.hpp from compiled C++: the
// worked value of gnx_align.h with two bases cut by min_baseq, and the header's "10 ref + 10 alt at q30" genotype from a pile built for it.
#include <cstdio>
#include <cstring>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

template <class F>
static bool refuses(F f) {
    try { f(); } catch (const std::exception &) { return true; }
    return false;
}

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    static_assert(sizeof(gnx_pile_genotype) == 48 && sizeof(gnx_geno_opts) == 24, "the layouts of gnx_align.h");
    // no pile: every entry refuses and writes nothing
    CHECK(gnx_pileup_close() == GNX_OK);
    int32_t tr = 7, mq = 7;
    int64_t bytes = 7;
    CHECK(gnx_pileup_qual_info(&tr, &mq, &bytes) == GNX_EINVAL && tr == 7 && mq == 7 && bytes == 7);
    CHECK(gnx_pileup_track_qualities(0) == GNX_EINVAL);
    CHECK(refuses([] { align::PileupGenotypes(); }));
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the call refuses like the align entries
        try { align::PileupOpen(0, 10); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(43);
    Seq genome(400);
    for (auto &x : genome) x = (dna::Base)(rng() % 4);
    const Seq a0 = dna::StringToBases("ACGTACGTAC"), b0 = dna::StringToBases("ACGAACTAC");
    std::copy(a0.begin(), a0.end(), genome.begin() + 100);
    const std::vector<align::Cigar> r0 = {{6, align::ColM}, {1, align::ColD}, {3, align::ColM}};
    if (gnx_set_reference(genome.data(), (int64_t)genome.size())) return 1;
    // the worked value: min_baseq 20 cuts the G at 102 (q10) and the T at 107 (q5)
    align::PileupOpen(0, 400);
    CHECK(gnx_pileup_qual_info(&tr, &mq, &bytes) == GNX_OK && tr == 0 && mq == 0 && bytes == 0);
    CHECK(refuses([&] { align::PileupAdd(mx, -600, -150, {b0}, {{30, 30, 10, 30, 40, 30, 5, 30, 30}}, {{100, 10}}, {0}, {r0}); })); // (a plain pile)
    CHECK(refuses([] { align::PileupGetQual(); }) && refuses([] { align::PileupGenotypes(); }));
    CHECK(gnx_pileup_track_qualities(94) == GNX_EINVAL && gnx_pileup_track_qualities(-1) == GNX_EINVAL);
    align::PileupTrackQualities(20);
    CHECK(gnx_pileup_qual_info(&tr, &mq, &bytes) == GNX_OK && tr == 1 && mq == 20 && bytes == 400 * 16 && align::PileupInfo().DeviceBytes == 400 * 56);
    CHECK(refuses([&] { align::PileupAdd(mx, -600, -150, {b0}, {{100, 10}}, {0}, {r0}); })); // (the plain entry on a quality pile)
    CHECK(align::PileupInfo().ReadsAdded == 0);
    align::PileupAdd(mx, -600, -150, {b0}, {{30, 30, 10, 30, 40, 30, 5, 30, 30}}, {{100, 10}}, {0}, {r0});
    CHECK(align::PileupInfo().ReadsAdded == 1);
    const auto rows = align::PileupGet(100, 10);
    const auto sums = align::PileupGetQual(100, 10);
    const int letter[10] = {0, 1, -1, 0, 0, 1, -1, -1, 0, 1}, qual[10] = {30, 30, 0, 30, 40, 30, 0, 0, 30, 30}; // (-1: nothing counted there)
    for (int k = 0; k < 10; k++) {
        gnx_pile exp;
        std::memset(&exp, 0, sizeof(exp));
        std::array<int32_t, 4> q = {0, 0, 0, 0};
        if (letter[k] >= 0) { exp.base[0][letter[k]] = 1; q[(size_t)letter[k]] = qual[k]; }
        if (k == 6) exp.del[0] = 1;
        CHECK(std::memcmp(&exp, &rows[(size_t)k], sizeof(exp)) == 0 && sums[(size_t)k] == q);
    }
    CHECK(refuses([] { align::PileupTrackQualities(0); })); // (reads have been added)
    // 10 ref + 10 alt bases at q30 at position 210: L = (34 770, 9 020, 38 070)
    align::PileupOpen(150, 200);
    align::PileupTrackQualities();
    Seq ref_read(genome.begin() + 200, genome.begin() + 240), alt_read(ref_read);
    alt_read[10] = (dna::Base)((alt_read[10] + 1) % 4);
    std::vector<Seq> reads;
    std::vector<std::vector<uint8_t>> quals;
    std::vector<std::pair<int64_t, int64_t>> windows;
    std::vector<uint8_t> strands;
    std::vector<std::vector<align::Cigar>> routes;
    for (int k = 0; k < 20; k++) {
        reads.push_back(k < 10 ? ref_read : alt_read);
        quals.push_back(std::vector<uint8_t>(40, 30));
        windows.push_back({200, 40});
        strands.push_back(k % 10 < 7 ? 0 : 1);
        routes.push_back({{40, align::ColM}});
    }
    align::PileupAdd(mx, -600, -150, reads, quals, windows, strands, routes);
    const auto g = align::PileupGenotypes();
    CHECK(g.size() == 1);
    CHECK(g[0].pos == 210 && g[0].gt == 1 && g[0].ref == genome[210] && g[0].alt == (genome[210] + 1) % 4 && g[0]._pad == 0);
    CHECK(g[0].pl[0] == 25750 && g[0].pl[1] == 0 && g[0].pl[2] == 29050 && g[0].gq == 25750 && g[0].qual == 25750);
    CHECK(g[0].depth == 20 && g[0].ref_count == 10 && g[0].alt_count == 10 && g[0].alt_fwd == 7);
    align::GenoOpts o;
    o.MinQual = 25751;
    CHECK(align::PileupGenotypes(o).empty());
    o.MinQual = 25750; o.MinDepth = 20;
    CHECK(align::PileupGenotypes(o).size() == 1);
    o.MinDepth = 21;
    CHECK(align::PileupGenotypes(o).empty());
    // open replaces the pile: tracking is off again; the pile belongs to the reference
    align::PileupOpen(0, 50);
    CHECK(gnx_pileup_qual_info(&tr, nullptr, &bytes) == GNX_OK && tr == 0 && bytes == 0);
    gnx_set_reference(nullptr, 0);
    CHECK(gnx_pileup_qual_info(nullptr, nullptr, nullptr) == GNX_EINVAL);
    std::printf("pile qual mirror ok%s\n", "");
    return 0;
}
