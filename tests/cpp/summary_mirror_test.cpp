// Summarize / SummarizeByOffset of include/gonomics_align.hpp from compiled C++: the routes AlignBatch returns are summarised and
// checked against a column-by-column restatement written here; the resident reference gives what the same bytes give.
#include <cstdio>
#include <random>

#include "gonomics_align.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using Seq = std::vector<dna::Base>;

// the definition of gnx_align.h on the expanded columns
static int restate(int mode, const align::ScoreMatrix &mx, int64_t go, int64_t ge, const Seq &a, const Seq &b, const std::vector<align::Cigar> &route,
                   const align::Summary &got) {
    std::vector<int> cols, types;
    for (const auto &c : route) for (int64_t k = 0; k < c.RunLength; k++) cols.push_back(c.Op);
    size_t i = 0, j = 0;
    int64_t match = 0, eq = 0, mm = 0;
    for (int c : cols) {
        if (c == align::ColM) { const bool e = a[i] == b[j]; types.push_back(e ? align::ColEq : align::ColX); match += mx[a[i]][b[j]]; (e ? eq : mm)++; i++; j++; }
        else if (c == align::ColI) { types.push_back(c); j++; }
        else { types.push_back(c); i++; }
    }
    size_t lead = 0, trail = 0;
    if (mode == GNX_AFFINE_GAP_LOCAL) {
        while (lead < cols.size() && cols[lead] == align::ColD) lead++;
        while (lead + trail < cols.size() && cols[cols.size() - 1 - trail] == align::ColD) trail++;
    }
    int64_t ins = 0, del = 0, runs = 0;
    int prev = -1;
    for (size_t k = lead; k + trail < cols.size(); k++) {
        if (cols[k] == align::ColI) ins++;
        if (cols[k] == align::ColD) del++;
        if (cols[k] != align::ColM && cols[k] != prev) runs++;
        prev = cols[k];
    }
    const bool affine = mode == GNX_AFFINE_GAP || mode == GNX_AFFINE_GAP_HIGHMEM || mode == GNX_AFFINE_GAP_LOCAL;
    const bool all_free = mode == GNX_AFFINE_GAP_LOCAL && !cols.empty() && lead == cols.size();
    std::vector<align::Cigar> x;
    for (int t : types) { if (!x.empty() && x.back().Op == t) x.back().RunLength++; else x.push_back(align::Cigar{1, (align::ColType)t}); }
    const gnx_aln_summary &s = got.S;
    CHECK(s.rescore == match + (affine ? go * runs + ge * (ins + del) : go * (ins + del)));
    CHECK(s.alpha_used == (int64_t)i && s.beta_used == (int64_t)j);
    CHECK(s.alpha_start == (all_free ? 0 : (int64_t)lead) && s.alpha_end == (all_free ? 0 : (int64_t)(i - trail)));
    CHECK(s.n_equal == eq && s.n_mismatch == mm && s.ins_bases == ins && s.del_bases == del && s.gap_runs == runs);
    CHECK(s.n_xops == (int64_t)x.size() && s._reserved == 0);
    CHECK(got.XCigar.size() == x.size());
    for (size_t k = 0; k < x.size(); k++) CHECK(got.XCigar[k].RunLength == x[k].RunLength && got.XCigar[k].Op == x[k].Op);
    return 0;
}

int main() {
    const auto &mx = align::HumanChimpTwoScoreMatrix();
    const Seq a0 = dna::StringToBases("ACGTACGTAC"), b0 = dna::StringToBases("ACGAACTAC");
    const std::vector<align::Cigar> r0 = {{6, align::ColM}, {1, align::ColD}, {3, align::ColM}};
    if (gnx_device_count() <= 0) {
        // no CPU fallback: the call refuses like the align entries
        try { align::Summarize(GNX_AFFINE_GAP_HIGHMEM, mx, -600, -150, {a0}, {b0}, {r0}); }
        catch (const std::exception &) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
        return 1;
    }
    {
        const auto s = align::Summarize(GNX_AFFINE_GAP_HIGHMEM, mx, -600, -150, {a0}, {b0}, {r0}, true);
        CHECK(s.size() == 1 && align::FormatXCigar(s[0].XCigar) == "3=1X2=1D3=" && align::FormatXCigar({}) == "*");
        if (restate(GNX_AFFINE_GAP_HIGHMEM, mx, -600, -150, a0, b0, r0, s[0])) return 1;
        CHECK(align::Summarize(GNX_AFFINE_GAP_HIGHMEM, mx, -600, -150, {a0}, {b0}, {r0})[0].XCigar.empty());
    }
    std::mt19937 rng(31);
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
        const std::vector<Seq> &alphas = local ? wins : reads, &betas = local ? reads : wins;
        std::vector<int64_t> sc; std::vector<std::vector<align::Cigar>> rt;
        align::AlignBatch(mode, mx, go, ge, 10000, 10000, alphas, betas, sc, rt);
        const auto got = align::Summarize(mode, mx, go, ge, alphas, betas, rt, true);
        CHECK(got.size() == reads.size());
        for (size_t k = 0; k < got.size(); k++) {
            if (restate(mode, mx, go, ge, alphas[k], betas[k], rt[k], got[k])) return 1;
            CHECK(got[k].S.rescore == sc[k]);
        }
        // the same windows from the resident reference
        if (gnx_set_reference(genome.data(), (int64_t)genome.size())) return 1;
        const auto res = align::SummarizeByOffset(mode, mx, go, ge, reads, windows, rt, true);
        gnx_set_reference(nullptr, 0);
        CHECK(res.size() == got.size());
        for (size_t k = 0; k < got.size(); k++) {
            CHECK(res[k].S.rescore == got[k].S.rescore && res[k].S.n_equal == got[k].S.n_equal && res[k].S.n_xops == got[k].S.n_xops && res[k].S.gap_runs == got[k].S.gap_runs);
            CHECK(align::FormatXCigar(res[k].XCigar) == align::FormatXCigar(got[k].XCigar));
        }
    }
    std::printf("summary mirror ok%s\n", "");
    return 0;
}
