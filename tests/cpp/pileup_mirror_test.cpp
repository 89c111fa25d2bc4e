// Pileup* of include/gonomics_align.hpp from compiled C++: the two worked values of gnx_align.h row by row, and one call of each kind
// from a pile built for it.
#include <cstdio>
#include <cstring>
#include <map>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

// rows [first, first + rows.size()) hold exactly `want`: position -> (plane, strand, slot) bumped once; plane 0 base, 1 del, 2 ins
struct Where { int plane, strand, slot; };
static bool holds(const std::vector<gnx_pile> &rows, int64_t first, const std::map<int64_t, Where> &want) {
    for (size_t k = 0; k < rows.size(); k++) {
        gnx_pile exp;
        std::memset(&exp, 0, sizeof(exp));
        const auto it = want.find(first + (int64_t)k);
        if (it != want.end()) {
            const Where &w = it->second;
            if (w.plane == 0) exp.base[w.strand][w.slot] = 1;
            else if (w.plane == 1) exp.del[w.strand] = 1;
            else exp.ins[w.strand] = 1;
        }
        if (std::memcmp(&exp, &rows[k], sizeof(exp)) != 0) { std::printf("row %lld differs\n", (long long)(first + (int64_t)k)); return false; }
    }
    return true;
}

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    static_assert(sizeof(gnx_pile) == 64 && sizeof(gnx_pile_call) == 24 && sizeof(gnx_pile_call_opts) == 24, "the layouts of gnx_align.h");
    // no pile: close is fine, everything else refuses
    CHECK(gnx_pileup_close() == GNX_OK);
    CHECK(gnx_pileup_info(nullptr, nullptr, nullptr, nullptr) == GNX_EINVAL);
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the call refuses like the align entries
        try { align::PileupOpen(0, 10); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(41);
    Seq genome(400);
    for (auto &x : genome) x = (dna::Base)(rng() % 4);
    const Seq a0 = dna::StringToBases("ACGTACGTAC"), b0 = dna::StringToBases("ACGAACTAC"), b1 = dna::StringToBases("TTTACG");
    std::copy(a0.begin(), a0.end(), genome.begin() + 100);
    const std::vector<align::Cigar> r0 = {{6, align::ColM}, {1, align::ColD}, {3, align::ColM}}, r1 = {{3, align::ColD}, {2, align::ColI}, {4, align::ColM}, {3, align::ColD}};
    if (gnx_set_reference(genome.data(), (int64_t)genome.size())) return 1;
    // worked value 1, strand 0, the whole reference as the region
    align::PileupOpen(0, 400);
    align::PileupAdd(mx, -600, -150, {b0}, {{100, 10}}, {0}, {r0});
    CHECK(holds(align::PileupGet(), 0, {{100, {0, 0, 0}}, {101, {0, 0, 1}}, {102, {0, 0, 2}}, {103, {0, 0, 0}}, {104, {0, 0, 0}}, {105, {0, 0, 1}}, {106, {1, 0, 0}},
                                        {107, {0, 0, 3}}, {108, {0, 0, 0}}, {109, {0, 0, 1}}}));
    CHECK(align::PileupInfo().ReadsAdded == 1 && align::PileupInfo().Len == 400 && align::PileupInfo().DeviceBytes == 400 * 56);
    // worked value 2, strand 1, a region that cuts it: open replaces
    align::PileupOpen(104, 50);
    align::PileupAdd(mx, -600, -150, {b1}, {{100, 10}}, {1}, {r1});
    CHECK(holds(align::PileupGet(), 104, {{104, {0, 1, 0}}, {105, {0, 1, 1}}, {106, {0, 1, 2}}}));
    CHECK(holds(align::PileupGet(2, 3), 106, {{106, {0, 1, 2}}}));
    for (const auto &c : align::PileupCalls()) CHECK(c.pos >= 104 && c.pos <= 106 && c.depth == 1 && c.count_fwd == 0); // (one reverse read: whatever it says, it says it there)
    // one call of each kind: four copies of a read with a substitution at 205, a deleted base at 220 and two inserted ones behind 239
    align::PileupOpen(0, 400);
    const std::vector<align::Cigar> r2 = {{20, align::ColM}, {1, align::ColD}, {19, align::ColM}, {2, align::ColI}, {20, align::ColM}};
    Seq rd(genome.begin() + 200, genome.begin() + 220);
    rd.insert(rd.end(), genome.begin() + 221, genome.begin() + 240);
    rd.push_back(2); rd.push_back(2);
    rd.insert(rd.end(), genome.begin() + 240, genome.begin() + 260);
    rd[5] = (dna::Base)((rd[5] + 1) % 4);
    align::PileupAdd(mx, -600, -150, {rd, rd, rd, rd, rd}, {{200, 60}, {200, 60}, {200, 60}, {200, 60}, {200, 60}}, {0, 1, 0, 0, 0}, {r2, r2, r2, r2, r2}, {1, 1, 1, 0, 1});
    CHECK(align::PileupInfo().ReadsAdded == 4);
    align::PileCallOpts o;
    o.MinAlt = 2; o.BothStrands = true;
    const auto calls = align::PileupCalls(o);
    CHECK(calls.size() == 3);
    CHECK(calls[0].pos == 205 && calls[0].kind == 0 && calls[0].ref == genome[205] && calls[0].alt == (genome[205] + 1) % 4 && calls[0].depth == 4 && calls[0].count == 4 && calls[0].count_fwd == 3);
    CHECK(calls[1].pos == 220 && calls[1].kind == 1 && calls[1].ref == genome[220] && calls[1].alt == 0xFF && calls[1].depth == 4 && calls[1].count == 4 && calls[1].count_fwd == 3);
    CHECK(calls[2].pos == 239 && calls[2].kind == 2 && calls[2].ref == genome[239] && calls[2].alt == 0xFF && calls[2].depth == 4 && calls[2].count == 4 && calls[2].count_fwd == 3);
    o.MinDepth = 5;
    CHECK(align::PileupCalls(o).empty());
    // the pile belongs to the reference
    gnx_set_reference(nullptr, 0);
    CHECK(gnx_pileup_info(nullptr, nullptr, nullptr, nullptr) == GNX_EINVAL);
    std::printf("pileup mirror ok%s\n", "");
    return 0;
}
