// MapBestPair of include/gonomics_align.hpp from compiled C++.  Without an argument: the call refuses without a GPU (exit 2) or runs a
// tiny pair (exit 0).  With a table file (written by tests/test_best_pair_cpp.py): runs the tables and prints every result, one line per
// read and per pair, for the Python side to compare with the ctypes call on the same tables.
//   file: min_insert max_insert unpaired_penalty gap_open gap_extend cigar n_reads target_len, the target's bases, then per read its
//   length, its bases, its number of candidates and (start len strand) of each -- whitespace-separated integers
#include <cstdio>
#include <fstream>

#include "gonomics_align.hpp"

using Seq = std::vector<dna::Base>;

static void print_result(const align::ReadPairs &res) {
    for (const auto &r : res.Reads) {
        std::printf("read %d %lld %lld %lld %lld %d %lld cand", (int)r.Hit.Best, (long long)r.Hit.Score, (long long)r.TargetStart, (long long)r.Hit.TargetEnd, (long long)r.WindowStart,
                    (int)r.HasSecond, (long long)r.SecondScore);
        for (size_t c = 0; c < r.Hit.CandScores.size(); c++) std::printf(" %lld %lld %lld", (long long)r.Hit.CandScores[c], (long long)r.CandStarts[c], (long long)r.CandEnds[c]);
        std::printf(" route");
        for (const auto &c : r.Hit.Route) std::printf(" %lld %d", (long long)c.RunLength, (int)c.Op);
        std::printf("\n");
    }
    for (size_t k = 0; k < res.Proper.size(); k++) std::printf("pair %d %lld\n", (int)res.Proper[k], (long long)res.Tlen[k]);
}

int main(int argc, char **argv) {
    const auto &mx = align::DefaultScoreMatrix();
    if (argc < 2) {
        const Seq target = dna::StringToBases("GGACGTACGTAATTGCAAACCGGTTACGATCGA");
        const std::vector<Seq> reads = {dna::StringToBases("ACGTACGT"), dna::StringToBases("CGATCG")};
        const std::vector<std::vector<align::RefCandidate>> cands = {{{0, 14, 0}}, {{20, 13, 1}}};
        try {
            const align::ReadPairs res = align::MapBestPair(mx, -400, -30, reads, cands, align::PairOpts{0, 100, 0}, true, &target);
            if (res.Reads.size() != 2 || res.Proper.size() != 1 || res.Reads[0].Hit.Best != 0 || res.Reads[1].Hit.Best != 0) return 1;
            print_result(res);
        } catch (const std::exception &e) {
            if (gnx_device_count() <= 0) { std::printf("no HIP device: %s\n", "skipping compute"); return 2; }
            std::printf("FAILED: %s\n", e.what());
            return 1;
        }
        return gnx_device_count() > 0 ? 0 : 1; // (no CPU fallback: without a device the call must have thrown)
    }
    std::ifstream in(argv[1]);
    long long lo, hi, pen, go, ge, cigar, n, tl, v;
    if (!(in >> lo >> hi >> pen >> go >> ge >> cigar >> n >> tl)) return 3;
    Seq target((size_t)tl);
    for (auto &b : target) { in >> v; b = (dna::Base)v; }
    std::vector<Seq> reads((size_t)n);
    std::vector<std::vector<align::RefCandidate>> cands((size_t)n);
    for (long long r = 0; r < n; r++) {
        long long len, k;
        in >> len;
        reads[(size_t)r].resize((size_t)len);
        for (auto &b : reads[(size_t)r]) { in >> v; b = (dna::Base)v; }
        in >> k;
        for (long long c = 0; c < k; c++) { long long s, l, st; in >> s >> l >> st; cands[(size_t)r].push_back(align::RefCandidate{s, l, (uint8_t)st}); }
    }
    if (!in) return 3;
    try {
        print_result(align::MapBestPair(mx, go, ge, reads, cands, align::PairOpts{lo, hi, pen}, cigar != 0, &target));
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
