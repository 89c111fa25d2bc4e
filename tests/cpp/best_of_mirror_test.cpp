// MapBestOf of include/gonomics_align.hpp from compiled C++: per read the first best candidate on either strand, with the score and
// route AlignBatch gives for that pair (the reverse complement taken on the host), every candidate's score and the locate twin's end.
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

static bool same(const std::vector<align::Cigar> &a, const std::vector<align::Cigar> &b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++) if (a[k].RunLength != b[k].RunLength || a[k].Op != b[k].Op) return false;
    return true;
}

// the flattened pair list through the existing entries: 0 on equality
static int check_against_twins(int mode, const align::ScoreMatrix &mx, int64_t go, int64_t ge, const std::vector<Seq> &reads,
                               const std::vector<std::vector<align::SeqCandidate>> &cands, const std::vector<align::BestOf> &got) {
    const bool local = mode == GNX_AFFINE_GAP_LOCAL;
    std::vector<Seq> alphas, betas;
    for (size_t r = 0; r < reads.size(); r++)
        for (const auto &cd : cands[r]) {
            Seq rd = reads[r];
            if (cd.Strand) dna::ReverseComplement(rd);
            alphas.push_back(local ? cd.Target : rd); betas.push_back(local ? rd : cd.Target);
        }
    std::vector<int64_t> sc; std::vector<std::vector<align::Cigar>> rt;
    align::AlignBatch(mode, mx, go, ge, 10000, 10000, alphas, betas, sc, rt);
    std::pair<std::vector<int64_t>, std::vector<int64_t>> loc;
    if (local) loc = align::LocateBatch(mx, go, ge, alphas, betas);
    CHECK(got.size() == reads.size());
    size_t at = 0;
    for (size_t r = 0; r < reads.size(); r++) {
        const size_t k = cands[r].size();
        CHECK(got[r].CandScores.size() == k);
        if (k == 0) { CHECK(got[r].Best == -1 && got[r].Score == 0 && got[r].Route.empty() && got[r].TargetEnd == 0); continue; }
        size_t b = 0;
        for (size_t x = 0; x < k; x++) { CHECK(got[r].CandScores[x] == sc[at + x]); if (sc[at + x] > sc[at + b]) b = x; }
        CHECK(got[r].Best == (int32_t)b);
        CHECK(got[r].Score == sc[at + b]);
        CHECK(same(got[r].Route, rt[at + b]));
        if (local) CHECK(got[r].TargetEnd == loc.second[at + b]);
        at += k;
    }
    return 0;
}

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the call refuses like the align entries
        try { align::MapBestOf(GNX_AFFINE_GAP, mx, -600, -150, {dna::StringToBases("ACGT")}, std::vector<std::vector<align::SeqCandidate>>{{{dna::StringToBases("ACGTT"), 0}}}); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    std::mt19937 rng(29);
    auto seq = [&](size_t n) { Seq v(n); for (auto &x : v) x = (dna::Base)(rng() % 4); return v; };
    Seq genome = seq(6000);
    std::vector<Seq> reads;
    std::vector<std::vector<align::SeqCandidate>> cands;
    for (int r = 0; r < 60; r++) {
        const size_t len = 20 + rng() % 180, at = rng() % (genome.size() - 700);
        Seq rd(genome.begin() + (long)at + 100, genome.begin() + (long)(at + 100 + len));
        const uint8_t strand = (uint8_t)(rng() % 2);
        if (strand) dna::ReverseComplement(rd); // the read as sequenced from the other strand: candidate strand 1 undoes it
        reads.push_back(rd);
        std::vector<align::SeqCandidate> cs;
        const int k = (int)(rng() % 5); // 0 .. 4 candidates
        for (int x = 0; x < k; x++) {
            const size_t o = x == 1 ? at : rng() % (genome.size() - 600), wl = 1 + rng() % 600;
            cs.push_back(align::SeqCandidate{Seq(genome.begin() + (long)o, genome.begin() + (long)(o + wl)), x == 1 ? strand : (uint8_t)(rng() % 2)});
        }
        cands.push_back(cs);
    }
    // 1: global affine, both strands, reads without candidates among them
    auto got = align::MapBestOf(GNX_AFFINE_GAP, mx, -600, -150, reads, cands);
    if (check_against_twins(GNX_AFFINE_GAP, mx, -600, -150, reads, cands, got)) return 1;
    // 2: the mapping mode (target = window, query = read) with the target end
    got = align::MapBestOf(GNX_AFFINE_GAP_LOCAL, mx, -600, -150, reads, cands);
    if (check_against_twins(GNX_AFFINE_GAP_LOCAL, mx, -600, -150, reads, cands, got)) return 1;
    bool inside = false;
    for (size_t r = 0; r < reads.size(); r++) if (got[r].Best >= 0) inside = inside || got[r].TargetEnd < (int64_t)cands[r][(size_t)got[r].Best].Target.size();
    CHECK(inside);
    // 3: ties go to the lowest index: a duplicated window, and a read that equals its own reverse complement on both strands
    const Seq pal = dna::StringToBases("ACGTACGT"), win = dna::StringToBases("TTACGTACGTGG");
    Seq pal_rc = pal;
    dna::ReverseComplement(pal_rc);
    CHECK(pal_rc == pal);
    std::vector<std::vector<align::SeqCandidate>> tie = {{{win, 0}, {win, 0}, {win, 1}}, {{win, 1}, {win, 0}}};
    for (int mode : {GNX_AFFINE_GAP, GNX_AFFINE_GAP_LOCAL}) {
        got = align::MapBestOf(mode, mx, -600, -150, {pal, pal}, tie);
        CHECK(got[0].Best == 0 && got[1].Best == 0);
        CHECK(got[0].CandScores[0] == got[0].CandScores[1] && got[0].CandScores[1] == got[0].CandScores[2]);
        if (check_against_twins(mode, mx, -600, -150, {pal, pal}, tie, got)) return 1;
    }
    // no CIGAR stage: the same winners and scores, no routes
    const auto bare = align::MapBestOf(GNX_AFFINE_GAP, mx, -600, -150, reads, cands, false);
    got = align::MapBestOf(GNX_AFFINE_GAP, mx, -600, -150, reads, cands);
    for (size_t r = 0; r < reads.size(); r++) CHECK(bare[r].Best == got[r].Best && bare[r].Score == got[r].Score && bare[r].Route.empty());
    bool threw = false;
    try { align::MapBestOf(GNX_AFFINE_GAP, mx, -600, -150, {Seq{0, 9, 1}}, std::vector<std::vector<align::SeqCandidate>>{{{win, 1}}}); } catch (const std::out_of_range &) { threw = true; }
    CHECK(threw);
    std::printf("best-of mirror ok\n");
    return 0;
}
