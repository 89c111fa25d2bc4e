// gonomics_align.hpp -- C++ host-side mirror of gonomics' `align` package API for the DP hot path, written above the
// C ABI (gnx_align.h).  The reference is Go (no Go toolchain in the build image), so the compiled-language host side
// is C++: same function names, argument order and meaning, and error behaviour as the Go functions:
//
//   align::AffineGap / AffineGap_customizeCheckersize      /root/reference/align/affineGap.go:59,73
//   align::ConstGap / ConstGap_customizeCheckersize        /root/reference/align/constGap.go:13,73
//   align::AffineGap_highMem / AffineGapLocal              /root/reference/align/affineGap_highMem.go:99,105
//   align::ConstGap_highMem                                /root/reference/align/constGap_highMem.go:11
//   align::AlignBatch (the batched loop of cmd/globalAlignmentAnchor.go:352-384 and the FIFO engine of
//                      affineGap_highMem.go:120-179: results in input order)
//   align::View / PrintCigar                               /root/reference/align/view.go:26-60
//   align::Cigar, ColM/ColI/ColD, score matrices           /root/reference/align/align.go:12-64
//
// Go panics become C++ exceptions: base >= 5 -> std::out_of_range ("index out of range"), empty input to a
// low-memory function (the Go code never terminates) -> std::invalid_argument, everything else std::runtime_error.
#ifndef GONOMICS_ALIGN_HPP
#define GONOMICS_ALIGN_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gnx_align.h"

namespace dna {
using Base = uint8_t; // /root/reference/dna/dna.go:5-21
enum : Base { A = 0, C = 1, G = 2, T = 3, N = 4, LowerA = 5, LowerC = 6, LowerG = 7, LowerT = 8, LowerN = 9, Gap = 10, Dot = 11, Nil = 12 };

inline std::vector<Base> StringToBases(const std::string &s) { // dna/convert.go:143-153
    std::vector<Base> out(s.size());
    for (size_t i = 0; i < s.size(); i++) {
        switch (s[i]) {
        case 'A': out[i] = A; break; case 'C': out[i] = C; break; case 'G': out[i] = G; break; case 'T': out[i] = T; break;
        case 'N': out[i] = N; break; case 'a': out[i] = LowerA; break; case 'c': out[i] = LowerC; break;
        case 'g': out[i] = LowerG; break; case 't': out[i] = LowerT; break; case 'n': out[i] = LowerN; break;
        case '-': out[i] = Gap; break; case '*': out[i] = Nil; break; case '.': out[i] = Dot; break;
        default: throw std::invalid_argument(std::string("Error: '") + s[i] + "' is an invalid base.");
        }
    }
    return out;
}
inline std::string BasesToString(const std::vector<Base> &b) { // dna/convert.go:178-187
    static const char tab[] = "ACGTNacgtn-.*";
    std::string s(b.size(), '?');
    for (size_t i = 0; i < b.size(); i++) { if (b[i] > Nil) throw std::out_of_range("index out of range"); s[i] = tab[b[i]]; }
    return s;
}
inline void AllToUpper(std::vector<Base> &b) { // dna/modify.go:60
    for (auto &x : b) if (x >= LowerA && x <= LowerN) x = (Base)(x - 5);
}
inline void ReverseComplement(std::vector<Base> &b) { // dna/modify.go:111 (in place; a byte beyond Nil stays what it is instead of panicking)
    static const Base comp[13] = {T, G, C, A, N, LowerT, LowerG, LowerC, LowerA, LowerN, Gap, Dot, Nil};
    std::reverse(b.begin(), b.end());
    for (auto &x : b) if (x <= Nil) x = comp[x];
}
} // namespace dna

namespace align {

using ColType = uint8_t;
constexpr ColType ColM = 0, ColI = 1, ColD = 2;
struct Cigar { int64_t RunLength; ColType Op; };
using ScoreMatrix = std::array<std::array<int64_t, 5>, 5>;

inline const ScoreMatrix &DefaultScoreMatrix() { static const ScoreMatrix m = {{{91, -114, -31, -123, -44}, {-114, 100, -125, -31, -43}, {-31, -125, 100, -114, -43}, {-123, -31, -114, 91, -44}, {-44, -43, -43, -44, -43}}}; return m; }
inline const ScoreMatrix &HoxD55ScoreMatrix() { static const ScoreMatrix m = {{{91, -114, -31, -123, 0}, {-114, 100, -125, -31, 0}, {-31, -125, 100, -114, 0}, {-123, -31, -114, 91, 0}, {0, 0, 0, 0, 0}}}; return m; }
inline const ScoreMatrix &MouseRatScoreMatrix() { return HoxD55ScoreMatrix(); }
inline const ScoreMatrix &HumanChimpTwoScoreMatrix() { static const ScoreMatrix m = {{{90, -330, -236, -356, -208}, {-330, 100, -318, -236, -196}, {-236, -318, 100, -330, -196}, {-356, -236, -330, 90, -208}, {-208, -196, -196, -208, -202}}}; return m; }

namespace detail {
inline gnx_params params(int mode, const ScoreMatrix &s, int64_t gapOpen, int64_t gapExtend, int64_t ci, int64_t cj) {
    gnx_params p{};
    p.mode = mode;
    for (int a = 0; a < 5; a++) for (int b = 0; b < 5; b++) p.scores[a * 5 + b] = s[a][b];
    p.gap_open = gapOpen; p.gap_extend = gapExtend; p.checkersize_i = ci; p.checkersize_j = cj;
    return p;
}
[[noreturn]] inline void raise(int rc) {
    const std::string msg = gnx_last_error();
    if (rc == GNX_EBASE) throw std::out_of_range("runtime error: index out of range: " + msg);
    if (rc == GNX_EEMPTY) throw std::invalid_argument(msg);
    throw std::runtime_error("gnx error " + std::to_string(rc) + ": " + msg);
}
inline std::pair<int64_t, std::vector<Cigar>> one(const gnx_params &p, const std::vector<dna::Base> &a, const std::vector<dna::Base> &b) {
    int64_t score = 0, n = 0;
    gnx_cigar *ops = nullptr;
    const int rc = gnx_align_pair(&p, a.data(), (int64_t)a.size(), b.data(), (int64_t)b.size(), &score, &ops, &n);
    if (rc) raise(rc);
    std::vector<Cigar> route((size_t)n);
    for (int64_t k = 0; k < n; k++) route[(size_t)k] = Cigar{ops[k].run_length, ops[k].op};
    gnx_free(ops);
    return {score, std::move(route)};
}
} // namespace detail

inline std::pair<int64_t, std::vector<Cigar>> AffineGap_customizeCheckersize(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, int checkersize_i, int checkersize_j) {
    return detail::one(detail::params(GNX_AFFINE_GAP, scores, gapOpen, gapExtend, checkersize_i, checkersize_j), alpha, beta);
}
inline std::pair<int64_t, std::vector<Cigar>> AffineGap(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    return AffineGap_customizeCheckersize(alpha, beta, scores, gapOpen, gapExtend, 10000, 10000);
}
inline std::pair<int64_t, std::vector<Cigar>> ConstGap_customizeCheckersize(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapPen, int checkersize_i, int checkersize_j) {
    return detail::one(detail::params(GNX_CONST_GAP, scores, gapPen, 0, checkersize_i, checkersize_j), alpha, beta);
}
inline std::pair<int64_t, std::vector<Cigar>> ConstGap(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapPen) {
    return ConstGap_customizeCheckersize(alpha, beta, scores, gapPen, 10000, 10000);
}
inline std::pair<int64_t, std::vector<Cigar>> AffineGap_highMem(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    return detail::one(detail::params(GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend, 10000, 10000), alpha, beta);
}
inline std::pair<int64_t, std::vector<Cigar>> AffineGapLocal(const std::vector<dna::Base> &target, const std::vector<dna::Base> &query, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    return detail::one(detail::params(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000), target, query);
}
inline std::pair<int64_t, std::vector<Cigar>> ConstGap_highMem(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapPen) {
    return detail::one(detail::params(GNX_CONST_GAP_HIGHMEM, scores, gapPen, 0, 10000, 10000), alpha, beta);
}

// TargetQueryPair + batched engine: GoAffineGapLocalEngine's channels become one call over a batch, FIFO order kept.
struct TargetQueryPair { std::vector<dna::Base> Target, Query; int64_t Score = 0; std::vector<Cigar> Cigar_; };

inline void AlignBatch(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, int checkersize_i, int checkersize_j,
                       const std::vector<std::vector<dna::Base>> &alphas, const std::vector<std::vector<dna::Base>> &betas,
                       std::vector<int64_t> &out_scores, std::vector<std::vector<Cigar>> &out_routes) {
    const int64_t n = (int64_t)alphas.size();
    std::vector<int64_t> aoff((size_t)n + 1, 0), boff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) { aoff[(size_t)k + 1] = aoff[(size_t)k] + (int64_t)alphas[(size_t)k].size(); boff[(size_t)k + 1] = boff[(size_t)k] + (int64_t)betas[(size_t)k].size(); }
    std::vector<dna::Base> acat((size_t)aoff[(size_t)n] + 1), bcat((size_t)boff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) {
        std::copy(alphas[(size_t)k].begin(), alphas[(size_t)k].end(), acat.begin() + aoff[(size_t)k]);
        std::copy(betas[(size_t)k].begin(), betas[(size_t)k].end(), bcat.begin() + boff[(size_t)k]);
    }
    const gnx_params p = detail::params(mode, scores, gapOpen, gapExtend, checkersize_i, checkersize_j);
    out_scores.assign((size_t)n, 0);
    gnx_cigar *ops = nullptr; int64_t *off = nullptr;
    const int rc = gnx_align_batch(&p, n, acat.data(), aoff.data(), bcat.data(), boff.data(), out_scores.data(), &ops, &off);
    if (rc) detail::raise(rc);
    out_routes.assign((size_t)n, {});
    for (int64_t k = 0; k < n; k++) for (int64_t x = off[k]; x < off[k + 1]; x++) out_routes[(size_t)k].push_back(Cigar{ops[x].run_length, ops[x].op});
    gnx_free(ops); gnx_free(off);
}

// ---- score-only calls (gnx_score_*; an extension: no Go function of the reference returns a score alone) ----
// The scores AlignBatch would return for these pairs, without their routes.
inline std::vector<int64_t> ScoreBatch(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend,
                                       const std::vector<std::vector<dna::Base>> &alphas, const std::vector<std::vector<dna::Base>> &betas) {
    const int64_t n = (int64_t)alphas.size();
    std::vector<int64_t> aoff((size_t)n + 1, 0), boff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) { aoff[(size_t)k + 1] = aoff[(size_t)k] + (int64_t)alphas[(size_t)k].size(); boff[(size_t)k + 1] = boff[(size_t)k] + (int64_t)betas[(size_t)k].size(); }
    std::vector<dna::Base> acat((size_t)aoff[(size_t)n] + 1), bcat((size_t)boff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) {
        std::copy(alphas[(size_t)k].begin(), alphas[(size_t)k].end(), acat.begin() + aoff[(size_t)k]);
        std::copy(betas[(size_t)k].begin(), betas[(size_t)k].end(), bcat.begin() + boff[(size_t)k]);
    }
    const gnx_params p = detail::params(mode, scores, gapOpen, gapExtend, 10000, 10000);
    std::vector<int64_t> out((size_t)std::max<int64_t>(n, 1), 0);
    const int rc = gnx_score_batch(&p, n, acat.data(), aoff.data(), bcat.data(), boff.data(), out.data());
    if (rc) detail::raise(rc);
    out.resize((size_t)n);
    return out;
}
inline int64_t AffineGapScore(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    return ScoreBatch(GNX_AFFINE_GAP, scores, gapOpen, gapExtend, {alpha}, {beta})[0];
}
inline int64_t ConstGapScore(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapPen) {
    return ScoreBatch(GNX_CONST_GAP, scores, gapPen, 0, {alpha}, {beta})[0];
}
inline int64_t AffineGapLocalScore(const std::vector<dna::Base> &target, const std::vector<dna::Base> &query, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    return ScoreBatch(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, {target}, {query})[0];
}

// ---- locate calls (gnx_locate_*; an extension) ----
// AffineGapLocal's score and target end for every (target, query) pair: {scores, targetEnds}; targetEnd = target length minus the
// trailing ColD run of the route AffineGapLocal returns (the target position just after the last aligned column).
inline std::pair<std::vector<int64_t>, std::vector<int64_t>> LocateBatch(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend,
                                                                         const std::vector<std::vector<dna::Base>> &targets, const std::vector<std::vector<dna::Base>> &queries) {
    const int64_t n = (int64_t)targets.size();
    std::vector<int64_t> toff((size_t)n + 1, 0), qoff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) { toff[(size_t)k + 1] = toff[(size_t)k] + (int64_t)targets[(size_t)k].size(); qoff[(size_t)k + 1] = qoff[(size_t)k] + (int64_t)queries[(size_t)k].size(); }
    std::vector<dna::Base> tcat((size_t)toff[(size_t)n] + 1), qcat((size_t)qoff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) {
        std::copy(targets[(size_t)k].begin(), targets[(size_t)k].end(), tcat.begin() + toff[(size_t)k]);
        std::copy(queries[(size_t)k].begin(), queries[(size_t)k].end(), qcat.begin() + qoff[(size_t)k]);
    }
    const gnx_params p = detail::params(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000);
    std::vector<int64_t> sc((size_t)std::max<int64_t>(n, 1), 0), end((size_t)std::max<int64_t>(n, 1), 0);
    const int rc = gnx_locate_batch(&p, n, tcat.data(), toff.data(), qcat.data(), qoff.data(), sc.data(), end.data());
    if (rc) detail::raise(rc);
    sc.resize((size_t)n); end.resize((size_t)n);
    return {sc, end};
}
// {score, targetEnd} of AffineGapLocal(target, query, ...) without its route
inline std::pair<int64_t, int64_t> AffineGapLocalEnd(const std::vector<dna::Base> &target, const std::vector<dna::Base> &query, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    const auto r = LocateBatch(scores, gapOpen, gapExtend, {target}, {query});
    return {r.first[0], r.second[0]};
}

// ---- span calls (gnx_locate_span_*; an extension) ----
// AffineGapLocal's score, target start and target end for every (target, query) pair; targetStart = the leading ColD run of the route
// AffineGapLocal returns (0 if it does not begin with one): the leftmost aligned target position.
struct Span { int64_t Score = 0, TargetStart = 0, TargetEnd = 0; };
inline std::vector<Span> LocateSpanBatch(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend,
                                         const std::vector<std::vector<dna::Base>> &targets, const std::vector<std::vector<dna::Base>> &queries) {
    const int64_t n = (int64_t)targets.size();
    std::vector<int64_t> toff((size_t)n + 1, 0), qoff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) { toff[(size_t)k + 1] = toff[(size_t)k] + (int64_t)targets[(size_t)k].size(); qoff[(size_t)k + 1] = qoff[(size_t)k] + (int64_t)queries[(size_t)k].size(); }
    std::vector<dna::Base> tcat((size_t)toff[(size_t)n] + 1), qcat((size_t)qoff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) {
        std::copy(targets[(size_t)k].begin(), targets[(size_t)k].end(), tcat.begin() + toff[(size_t)k]);
        std::copy(queries[(size_t)k].begin(), queries[(size_t)k].end(), qcat.begin() + qoff[(size_t)k]);
    }
    const gnx_params p = detail::params(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000);
    std::vector<int64_t> sc((size_t)std::max<int64_t>(n, 1), 0), start((size_t)std::max<int64_t>(n, 1), 0), end((size_t)std::max<int64_t>(n, 1), 0);
    const int rc = gnx_locate_span_batch(&p, n, tcat.data(), toff.data(), qcat.data(), qoff.data(), sc.data(), start.data(), end.data());
    if (rc) detail::raise(rc);
    std::vector<Span> out((size_t)n);
    for (int64_t k = 0; k < n; k++) { out[(size_t)k].Score = sc[(size_t)k]; out[(size_t)k].TargetStart = start[(size_t)k]; out[(size_t)k].TargetEnd = end[(size_t)k]; }
    return out;
}
// {score, targetStart, targetEnd} of AffineGapLocal(target, query, ...) without its route
inline Span AffineGapLocalSpan(const std::vector<dna::Base> &target, const std::vector<dna::Base> &query, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend) {
    return LocateSpanBatch(scores, gapOpen, gapExtend, {target}, {query})[0];
}

// ---- best of K on both strands (gnx_best_of_*; an extension) ----
// A read against candidate windows on either strand: per read the FIRST best candidate, its score and route, every candidate's score
// and, for GNX_AFFINE_GAP_LOCAL, the target end.  Global modes: alpha = the read (strand 1: its reverse complement), beta = the
// window; GNX_AFFINE_GAP_LOCAL: target = the window, query = the read.  A read without candidates gets Best = -1 and nothing else.
struct RefCandidate { int64_t Start, Len; uint8_t Strand; };                  // a window of the resident reference (gnx_set_reference)
struct SeqCandidate { std::vector<dna::Base> Target; uint8_t Strand; };       // a window given as bases
struct BestOf { int32_t Best = -1; int64_t Score = 0, TargetEnd = 0; std::vector<Cigar> Route; std::vector<int64_t> CandScores; };
namespace detail {
inline std::vector<BestOf> best_of(const gnx_params &p, const std::vector<std::vector<dna::Base>> &reads, const std::vector<dna::Base> *tcat,
                                   const std::vector<int64_t> &coff, const std::vector<int64_t> &cstart, const std::vector<int64_t> &clen, const std::vector<uint8_t> &cstrand, bool cigar) {
    const int64_t n = (int64_t)reads.size();
    std::vector<int64_t> roff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) roff[(size_t)k + 1] = roff[(size_t)k] + (int64_t)reads[(size_t)k].size();
    std::vector<dna::Base> rcat((size_t)roff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) std::copy(reads[(size_t)k].begin(), reads[(size_t)k].end(), rcat.begin() + roff[(size_t)k]);
    const size_t nn = (size_t)std::max<int64_t>(n, 1), nc = std::max<size_t>(cstart.size(), 1);
    std::vector<int32_t> best(nn, -1);
    std::vector<int64_t> sc(nn, 0), end(nn, 0), cand(nc, 0);
    const bool local = p.mode == GNX_AFFINE_GAP_LOCAL;
    gnx_cigar *ops = nullptr; int64_t *off = nullptr;
    const int rc = tcat ? gnx_best_of_windows(&p, n, rcat.data(), roff.data(), tcat->data(), (int64_t)tcat->size(), coff.data(), cstart.data(), clen.data(), cstrand.data(), best.data(), sc.data(),
                                              local ? end.data() : nullptr, cand.data(), cigar ? &ops : nullptr, cigar ? &off : nullptr)
                        : gnx_best_of_by_offset(&p, n, rcat.data(), roff.data(), coff.data(), cstart.data(), clen.data(), cstrand.data(), best.data(), sc.data(), local ? end.data() : nullptr, cand.data(),
                                                cigar ? &ops : nullptr, cigar ? &off : nullptr);
    if (rc) raise(rc);
    std::vector<BestOf> out((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        BestOf &b = out[(size_t)k];
        b.Best = best[(size_t)k]; b.Score = sc[(size_t)k]; b.TargetEnd = end[(size_t)k];
        b.CandScores.assign(cand.begin() + coff[(size_t)k], cand.begin() + coff[(size_t)k + 1]);
        for (int64_t x = cigar ? off[k] : 0; cigar && x < off[k + 1]; x++) b.Route.push_back(Cigar{ops[x].run_length, ops[x].op});
    }
    if (cigar) { gnx_free(ops); gnx_free(off); }
    return out;
}
} // namespace detail
inline std::vector<BestOf> MapBestOf(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                                     const std::vector<std::vector<SeqCandidate>> &candidates, bool cigar = true) {
    std::vector<int64_t> coff(reads.size() + 1, 0), cstart, clen;
    std::vector<uint8_t> cstrand;
    std::vector<dna::Base> tcat;
    for (size_t r = 0; r < reads.size(); r++) {
        for (const auto &cd : candidates[r]) {
            cstart.push_back((int64_t)tcat.size()); clen.push_back((int64_t)cd.Target.size()); cstrand.push_back(cd.Strand);
            tcat.insert(tcat.end(), cd.Target.begin(), cd.Target.end());
        }
        coff[r + 1] = (int64_t)cstart.size();
    }
    cstart.push_back(0); clen.push_back(0); cstrand.push_back(0); // (data() of an empty vector may be null)
    return detail::best_of(detail::params(mode, scores, gapOpen, gapExtend, 10000, 10000), reads, &tcat, coff, cstart, clen, cstrand, cigar);
}
inline std::vector<BestOf> MapBestOf(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                                     const std::vector<std::vector<RefCandidate>> &candidates, bool cigar = true) {
    std::vector<int64_t> coff(reads.size() + 1, 0), cstart, clen;
    std::vector<uint8_t> cstrand;
    for (size_t r = 0; r < reads.size(); r++) {
        for (const auto &cd : candidates[r]) { cstart.push_back(cd.Start); clen.push_back(cd.Len); cstrand.push_back(cd.Strand); }
        coff[r + 1] = (int64_t)cstart.size();
    }
    cstart.push_back(0); clen.push_back(0); cstrand.push_back(0);
    return detail::best_of(detail::params(mode, scores, gapOpen, gapExtend, 10000, 10000), reads, nullptr, coff, cstart, clen, cstrand, cigar);
}

// ---- candidates by seed votes on the resident reference, and reads in / placements out (gnx_reference_index_build, gnx_seed_candidates) ----
struct SeedVoteOpts { int32_t MaxOcc = 64, Bin = 32, Pad = 16, MaxCand = 4, MinVotes = 2; };
struct VotedCandidate { int64_t Start, Len; uint8_t Strand; int32_t Votes; };
struct Mapped { BestOf Hit; int64_t WindowStart = 0; uint8_t Strand = 0; }; // the winner's window start: add Hit.TargetEnd (or the route's leading D run) to it
inline void ReferenceIndexBuild(int seedLen, int seedStep = 1) { const int rc = gnx_reference_index_build(seedLen, seedStep); if (rc) detail::raise(rc); }
inline std::vector<std::vector<VotedCandidate>> SeedCandidates(const std::vector<std::vector<dna::Base>> &reads, const SeedVoteOpts &o = SeedVoteOpts()) {
    const int64_t n = (int64_t)reads.size();
    std::vector<int64_t> roff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) roff[(size_t)k + 1] = roff[(size_t)k] + (int64_t)reads[(size_t)k].size();
    std::vector<dna::Base> rcat((size_t)roff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) std::copy(reads[(size_t)k].begin(), reads[(size_t)k].end(), rcat.begin() + roff[(size_t)k]);
    gnx_seed_vote_opts vo = {o.MaxOcc, o.Bin, o.Pad, o.MaxCand, o.MinVotes, {0, 0, 0}};
    int64_t *coff = nullptr, *cstart = nullptr, *clen = nullptr; uint8_t *cstrand = nullptr; int32_t *cvotes = nullptr;
    const int rc = gnx_seed_candidates(&vo, n, rcat.data(), roff.data(), &coff, &cstart, &clen, &cstrand, &cvotes);
    if (rc) detail::raise(rc);
    std::vector<std::vector<VotedCandidate>> out((size_t)n);
    for (int64_t k = 0; k < n; k++)
        for (int64_t x = coff[k]; x < coff[k + 1]; x++) out[(size_t)k].push_back(VotedCandidate{cstart[x], clen[x], cstrand[x], cvotes[x]});
    gnx_free(coff); gnx_free(cstart); gnx_free(clen); gnx_free(cstrand); gnx_free(cvotes);
    return out;
}
inline std::vector<Mapped> MapReads(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                                    const SeedVoteOpts &o = SeedVoteOpts(), bool cigar = true) {
    const std::vector<std::vector<VotedCandidate>> voted = SeedCandidates(reads, o);
    std::vector<std::vector<RefCandidate>> cands(reads.size());
    for (size_t r = 0; r < reads.size(); r++) for (const auto &v : voted[r]) cands[r].push_back(RefCandidate{v.Start, v.Len, v.Strand});
    std::vector<BestOf> best = MapBestOf(mode, scores, gapOpen, gapExtend, reads, cands, cigar);
    std::vector<Mapped> out(reads.size());
    for (size_t r = 0; r < reads.size(); r++) {
        out[r].Hit = std::move(best[r]);
        if (out[r].Hit.Best >= 0) { out[r].WindowStart = cands[r][(size_t)out[r].Hit.Best].Start; out[r].Strand = cands[r][(size_t)out[r].Hit.Best].Strand; }
    }
    return out;
}

// ---- best proper pair (gnx_best_pair_*; an extension): reads[2k] and reads[2k + 1] are mates and are placed together ----
// Mode GNX_AFFINE_GAP_LOCAL.  Per read a BestOf plus the alignment's span relative to the chosen window (TargetStart, Hit.TargetEnd), the
// window's start in the caller's coordinates and the best score among the read's other candidates (HasSecond = false: none).  Per pair:
// Proper and Tlen (0 when not proper).  gnx_align.h states the selection rule.
struct PairOpts { int64_t MinInsert = 0, MaxInsert = 0, UnpairedPenalty = 0; };
struct PairedRead { BestOf Hit; int64_t TargetStart = 0, WindowStart = 0, SecondScore = 0; bool HasSecond = false; std::vector<int64_t> CandStarts, CandEnds; };
struct ReadPairs { std::vector<PairedRead> Reads; std::vector<uint8_t> Proper; std::vector<int64_t> Tlen; };
namespace detail {
inline ReadPairs best_pair(const gnx_params &p, const PairOpts &o, const std::vector<std::vector<dna::Base>> &reads, const std::vector<dna::Base> *tcat,
                           const std::vector<int64_t> &coff, const std::vector<int64_t> &cstart, const std::vector<int64_t> &clen, const std::vector<uint8_t> &cstrand, bool cigar) {
    const int64_t n = (int64_t)reads.size();
    std::vector<int64_t> roff((size_t)n + 1, 0);
    for (int64_t k = 0; k < n; k++) roff[(size_t)k + 1] = roff[(size_t)k] + (int64_t)reads[(size_t)k].size();
    std::vector<dna::Base> rcat((size_t)roff[(size_t)n] + 1);
    for (int64_t k = 0; k < n; k++) std::copy(reads[(size_t)k].begin(), reads[(size_t)k].end(), rcat.begin() + roff[(size_t)k]);
    const size_t nn = (size_t)std::max<int64_t>(n, 1), nc = std::max<size_t>(cstart.size(), 1);
    std::vector<int32_t> best(nn, -1);
    std::vector<int64_t> sc(nn, 0), start(nn, 0), end(nn, 0), second(nn, 0), tlen(nn, 0), cs(nc, 0), cb(nc, 0), ce(nc, 0);
    std::vector<uint8_t> proper(nn, 0);
    const gnx_pair_opts po = {o.MinInsert, o.MaxInsert, o.UnpairedPenalty, 0};
    gnx_cigar *ops = nullptr; int64_t *off = nullptr;
    const int rc = tcat ? gnx_best_pair_windows(&p, &po, n, rcat.data(), roff.data(), tcat->data(), (int64_t)tcat->size(), coff.data(), cstart.data(), clen.data(), cstrand.data(), best.data(),
                                                sc.data(), start.data(), end.data(), second.data(), proper.data(), tlen.data(), cs.data(), cb.data(), ce.data(), cigar ? &ops : nullptr, cigar ? &off : nullptr)
                        : gnx_best_pair_by_offset(&p, &po, n, rcat.data(), roff.data(), coff.data(), cstart.data(), clen.data(), cstrand.data(), best.data(),
                                                  sc.data(), start.data(), end.data(), second.data(), proper.data(), tlen.data(), cs.data(), cb.data(), ce.data(), cigar ? &ops : nullptr, cigar ? &off : nullptr);
    if (rc) raise(rc);
    ReadPairs out;
    out.Reads.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        PairedRead &r = out.Reads[(size_t)k];
        const int64_t c0 = coff[(size_t)k], c1 = coff[(size_t)k + 1];
        r.Hit.Best = best[(size_t)k]; r.Hit.Score = sc[(size_t)k]; r.Hit.TargetEnd = end[(size_t)k]; r.TargetStart = start[(size_t)k];
        r.Hit.CandScores.assign(cs.begin() + c0, cs.begin() + c1);
        r.CandStarts.assign(cb.begin() + c0, cb.begin() + c1);
        r.CandEnds.assign(ce.begin() + c0, ce.begin() + c1);
        if (r.Hit.Best >= 0) r.WindowStart = cstart[(size_t)(c0 + r.Hit.Best)];
        r.HasSecond = second[(size_t)k] != INT64_MIN;
        r.SecondScore = r.HasSecond ? second[(size_t)k] : 0;
        for (int64_t x = cigar ? off[k] : 0; cigar && x < off[k + 1]; x++) r.Hit.Route.push_back(Cigar{ops[x].run_length, ops[x].op});
    }
    out.Proper.assign(proper.begin(), proper.begin() + n / 2);
    out.Tlen.assign(tlen.begin(), tlen.begin() + n / 2);
    if (cigar) { gnx_free(ops); gnx_free(off); }
    return out;
}
} // namespace detail
// candidates: windows of the resident reference or, with target given, of that sequence
inline ReadPairs MapBestPair(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                             const std::vector<std::vector<RefCandidate>> &candidates, const PairOpts &o, bool cigar = true, const std::vector<dna::Base> *target = nullptr) {
    std::vector<int64_t> coff(reads.size() + 1, 0), cstart, clen;
    std::vector<uint8_t> cstrand;
    for (size_t r = 0; r < reads.size(); r++) {
        for (const auto &cd : candidates[r]) { cstart.push_back(cd.Start); clen.push_back(cd.Len); cstrand.push_back(cd.Strand); }
        coff[r + 1] = (int64_t)cstart.size();
    }
    cstart.push_back(0); clen.push_back(0); cstrand.push_back(0); // (data() of an empty vector may be null)
    return detail::best_pair(detail::params(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000), o, reads, target, coff, cstart, clen, cstrand, cigar);
}
// mate pairs in, placements out: SeedCandidates over all mates, then MapBestPair on its tables (WindowStart: a position of the resident reference)
inline ReadPairs MapReadPairs(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads, const PairOpts &o,
                              const SeedVoteOpts &vo = SeedVoteOpts(), bool cigar = true) {
    const std::vector<std::vector<VotedCandidate>> voted = SeedCandidates(reads, vo);
    std::vector<std::vector<RefCandidate>> cands(reads.size());
    for (size_t r = 0; r < reads.size(); r++) for (const auto &v : voted[r]) cands[r].push_back(RefCandidate{v.Start, v.Len, v.Strand});
    return MapBestPair(scores, gapOpen, gapExtend, reads, cands, o, cigar);
}

// ---- alignment summaries (gnx_summarize_*, an extension): what is IN finished alignments -- identities, substitutions, gap bases and
// runs, the column re-score, the =/X form of the route (ops ColEq / ColX in place of ColM; only with xcigar).  gnx_align.h defines each field.
constexpr ColType ColEq = GNX_XCOL_EQ, ColX = GNX_XCOL_X;
struct Summary { gnx_aln_summary S{}; std::vector<Cigar> XCigar; };
namespace detail {
inline void flatten(const std::vector<std::vector<dna::Base>> &seqs, std::vector<dna::Base> &cat, std::vector<int64_t> &off) {
    off.assign(seqs.size() + 1, 0);
    for (size_t k = 0; k < seqs.size(); k++) { cat.insert(cat.end(), seqs[k].begin(), seqs[k].end()); off[k + 1] = (int64_t)cat.size(); }
    cat.push_back(0); // (data() of an empty vector may be null)
}
// by_offset: betas is unused, windows = (start, len) of the resident reference
inline std::vector<Summary> summarize(const gnx_params &p, const std::vector<std::vector<dna::Base>> &alphas, const std::vector<std::vector<dna::Base>> *betas,
                                      const std::vector<std::pair<int64_t, int64_t>> *windows, const std::vector<std::vector<Cigar>> &routes, bool xcigar) {
    const int64_t n = (int64_t)routes.size();
    std::vector<dna::Base> acat, bcat;
    std::vector<int64_t> aoff, boff, ooff((size_t)n + 1, 0), ws, wl;
    std::vector<gnx_cigar> ops;
    flatten(alphas, acat, aoff);
    if (betas) flatten(*betas, bcat, boff);
    else for (const auto &w : *windows) { ws.push_back(w.first); wl.push_back(w.second); }
    ws.push_back(0); wl.push_back(0);
    for (int64_t k = 0; k < n; k++) {
        for (const Cigar &c : routes[(size_t)k]) { gnx_cigar g{}; g.run_length = c.RunLength; g.op = c.Op; ops.push_back(g); }
        ooff[(size_t)k + 1] = (int64_t)ops.size();
    }
    ops.push_back(gnx_cigar{});
    std::vector<gnx_aln_summary> out((size_t)n + 1);
    gnx_cigar *xops = nullptr;
    int64_t *xoff = nullptr;
    const int rc = betas ? gnx_summarize_batch(&p, n, acat.data(), aoff.data(), bcat.data(), boff.data(), ops.data(), ooff.data(), out.data(), xcigar ? &xops : nullptr, xcigar ? &xoff : nullptr)
                         : gnx_summarize_batch_by_offset(&p, n, acat.data(), aoff.data(), ws.data(), wl.data(), ops.data(), ooff.data(), out.data(), xcigar ? &xops : nullptr, xcigar ? &xoff : nullptr);
    if (rc) raise(rc);
    std::vector<Summary> res((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        res[(size_t)k].S = out[(size_t)k];
        if (xcigar) for (int64_t x = xoff[k]; x < xoff[k + 1]; x++) res[(size_t)k].XCigar.push_back(Cigar{xops[x].run_length, xops[x].op});
    }
    if (xcigar) { gnx_free(xops); gnx_free(xoff); }
    return res;
}
} // namespace detail
inline std::vector<Summary> Summarize(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &alphas,
                                      const std::vector<std::vector<dna::Base>> &betas, const std::vector<std::vector<Cigar>> &routes, bool xcigar = false) {
    return detail::summarize(detail::params(mode, scores, gapOpen, gapExtend, 10000, 10000), alphas, &betas, nullptr, routes, xcigar);
}
// reads against windows (start, len) of the resident reference, in MapBestOf's roles; a strand-1 winner's read goes in reverse-complemented
inline std::vector<Summary> SummarizeByOffset(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                                              const std::vector<std::pair<int64_t, int64_t>> &windows, const std::vector<std::vector<Cigar>> &routes, bool xcigar = false) {
    return detail::summarize(detail::params(mode, scores, gapOpen, gapExtend, 10000, 10000), reads, nullptr, &windows, routes, xcigar);
}
inline std::string FormatXCigar(const std::vector<Cigar> &route) { // e.g. "12=1X30=2D5=" ("*" for an empty one)
    std::string s;
    for (const Cigar &c : route) s += std::to_string(c.RunLength) + "MID=X"[c.Op];
    return s.empty() ? "*" : s;
}

// ---- MD strings (gnx_md_*, an extension) and the library's MAPQ rule (gnx_mapq_batch).  alphas[k] is the DESCRIBED side: the reference of
// SAM's MD:Z tag, whose letters stand under every substitution and deletion ("3T2^G3").  gnx_align.h defines both.
namespace detail {
// by_offset: alphas = the reads (the queries), betas unused, windows = (start, len) of the resident reference (the described side)
inline std::vector<std::string> md_tags(const gnx_params &p, const std::vector<std::vector<dna::Base>> &alphas, const std::vector<std::vector<dna::Base>> *betas,
                                        const std::vector<std::pair<int64_t, int64_t>> *windows, const std::vector<std::vector<Cigar>> &routes) {
    const int64_t n = (int64_t)routes.size();
    std::vector<dna::Base> acat, bcat;
    std::vector<int64_t> aoff, boff, ooff((size_t)n + 1, 0), ws, wl;
    std::vector<gnx_cigar> ops;
    flatten(alphas, acat, aoff);
    if (betas) flatten(*betas, bcat, boff);
    else for (const auto &w : *windows) { ws.push_back(w.first); wl.push_back(w.second); }
    ws.push_back(0); wl.push_back(0);
    for (int64_t k = 0; k < n; k++) {
        for (const Cigar &c : routes[(size_t)k]) { gnx_cigar g{}; g.run_length = c.RunLength; g.op = c.Op; ops.push_back(g); }
        ooff[(size_t)k + 1] = (int64_t)ops.size();
    }
    ops.push_back(gnx_cigar{});
    char *md = nullptr;
    int64_t *off = nullptr;
    const int rc = betas ? gnx_md_batch(&p, n, acat.data(), aoff.data(), bcat.data(), boff.data(), ops.data(), ooff.data(), &md, &off)
                         : gnx_md_batch_by_offset(&p, n, acat.data(), aoff.data(), ws.data(), wl.data(), ops.data(), ooff.data(), &md, &off);
    if (rc) raise(rc);
    std::vector<std::string> res((size_t)n);
    for (int64_t k = 0; k < n; k++) res[(size_t)k].assign(md + off[k], md + off[k + 1]);
    gnx_free(md); gnx_free(off);
    return res;
}
} // namespace detail
inline std::vector<std::string> MDTags(int mode, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &alphas,
                                       const std::vector<std::vector<dna::Base>> &betas, const std::vector<std::vector<Cigar>> &routes) {
    return detail::md_tags(detail::params(mode, scores, gapOpen, gapExtend, 10000, 10000), alphas, &betas, nullptr, routes);
}
// reads (queries, in the orientation they were aligned in) against windows (start, len) of the resident reference; GNX_AFFINE_GAP_LOCAL
inline std::vector<std::string> MDTagsByOffset(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                                               const std::vector<std::pair<int64_t, int64_t>> &windows, const std::vector<std::vector<Cigar>> &routes) {
    return detail::md_tags(detail::params(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000), reads, nullptr, &windows, routes);
}
// secondScores[r] = INT64_MIN: read r has no other candidate
inline std::vector<int> Mapq(const std::vector<int64_t> &scores, const std::vector<int64_t> &secondScores) {
    if (scores.size() != secondScores.size()) detail::raise(GNX_EINVAL);
    std::vector<uint8_t> q(scores.size() + 1);
    const int rc = gnx_mapq_batch((int64_t)scores.size(), scores.data(), secondScores.data(), q.data());
    if (rc) detail::raise(rc);
    return std::vector<int>(q.begin(), q.end() - 1);
}

// ---- the pile of the resident reference (gnx_pileup_*, an extension): per-position counts of placed reads and the calls they give.
// One pile per process, owned by the reference; gnx_align.h defines what is counted and the rule of the calls.
struct PileInfo { int64_t Start = 0, Len = 0, ReadsAdded = 0, DeviceBytes = 0; };
struct PileCallOpts { int MinDepth = 1, MinAlt = 1, FracNum = 1, FracDen = 2; bool BothStrands = false; };
inline void PileupOpen(int64_t start, int64_t length) { const int rc = gnx_pileup_open(start, length); if (rc) detail::raise(rc); }
inline void PileupClose() { const int rc = gnx_pileup_close(); if (rc) detail::raise(rc); }
inline PileInfo PileupInfo() {
    PileInfo i;
    const int rc = gnx_pileup_info(&i.Start, &i.Len, &i.ReadsAdded, &i.DeviceBytes);
    if (rc) detail::raise(rc);
    return i;
}
// reads (in the orientation they were aligned in) against windows (start, len) of the resident reference; strands[k] picks the counter;
// use: empty = all, else use[k] == 0 leaves pair k out.  GNX_AFFINE_GAP_LOCAL.
namespace detail {
// quals == nullptr: gnx_pileup_add_by_offset; else gnx_pileup_add_by_offset_qual with one raw Phred quality per read base
inline void pile_add(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                     const std::vector<std::vector<uint8_t>> *quals, const std::vector<std::pair<int64_t, int64_t>> &windows, const std::vector<uint8_t> &strands,
                     const std::vector<std::vector<Cigar>> &routes, const std::vector<uint8_t> &use) {
    const int64_t n = (int64_t)routes.size();
    if ((int64_t)reads.size() != n || (int64_t)windows.size() != n || (int64_t)strands.size() != n || (!use.empty() && (int64_t)use.size() != n)) detail::raise(GNX_EINVAL);
    std::vector<uint8_t> qcat;
    if (quals) {
        if ((int64_t)quals->size() != n) detail::raise(GNX_EINVAL);
        for (int64_t k = 0; k < n; k++) {
            if ((*quals)[(size_t)k].size() != reads[(size_t)k].size()) detail::raise(GNX_EINVAL);
            qcat.insert(qcat.end(), (*quals)[(size_t)k].begin(), (*quals)[(size_t)k].end());
        }
        qcat.push_back(0);
    }
    const gnx_params p = detail::params(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000);
    std::vector<dna::Base> cat;
    std::vector<int64_t> off, ooff((size_t)n + 1, 0), ws, wl;
    std::vector<gnx_cigar> ops;
    std::vector<uint8_t> st(strands);
    detail::flatten(reads, cat, off);
    for (const auto &w : windows) { ws.push_back(w.first); wl.push_back(w.second); }
    ws.push_back(0); wl.push_back(0); st.push_back(0);
    for (int64_t k = 0; k < n; k++) {
        for (const Cigar &c : routes[(size_t)k]) { gnx_cigar g{}; g.run_length = c.RunLength; g.op = c.Op; ops.push_back(g); }
        ooff[(size_t)k + 1] = (int64_t)ops.size();
    }
    ops.push_back(gnx_cigar{});
    const uint8_t *u = use.empty() ? nullptr : use.data();
    const int rc = quals ? gnx_pileup_add_by_offset_qual(&p, n, cat.data(), off.data(), ws.data(), wl.data(), st.data(), ops.data(), ooff.data(), u, qcat.data())
                         : gnx_pileup_add_by_offset(&p, n, cat.data(), off.data(), ws.data(), wl.data(), st.data(), ops.data(), ooff.data(), u);
    if (rc) detail::raise(rc);
}
} // namespace detail
inline void PileupAdd(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                      const std::vector<std::pair<int64_t, int64_t>> &windows, const std::vector<uint8_t> &strands, const std::vector<std::vector<Cigar>> &routes,
                      const std::vector<uint8_t> &use = {}) {
    detail::pile_add(scores, gapOpen, gapExtend, reads, nullptr, windows, strands, routes, use);
}
inline std::vector<gnx_pile> PileupGet(int64_t first = 0, int64_t count = -1) {
    if (count < 0) count = PileupInfo().Len - first;
    std::vector<gnx_pile> rows((size_t)(count > 0 ? count : 0) + 1);
    const int rc = gnx_pileup_get(first, count, rows.data());
    if (rc) detail::raise(rc);
    rows.pop_back();
    return rows;
}
inline std::vector<gnx_pile_call> PileupCalls(const PileCallOpts &o = PileCallOpts()) {
    const gnx_pile_call_opts co = {o.MinDepth, o.MinAlt, o.FracNum, o.FracDen, o.BothStrands ? 1 : 0, 0};
    gnx_pile_call *calls = nullptr;
    int64_t n = 0;
    const int rc = gnx_pileup_calls(&co, &calls, &n);
    if (rc) detail::raise(rc);
    std::vector<gnx_pile_call> res(calls, calls + n);
    gnx_free(calls);
    return res;
}

// base qualities in the pile and diploid SNP genotypes (gnx_pileup_track_qualities .. gnx_pileup_genotypes): the open pile, still empty,
// sums the qualities of what it counts and leaves out bases below minBaseQ; its reads then come with quals[k][j] = the raw Phred quality of
// reads[k][j] (the same orientation); the rule of the genotypes, in centi-Phred, is gnx_align.h's
struct GenoOpts { int MinDepth = 1, MinQual = 0, PriorHet = 3000, PriorHom = 3300; };
inline void PileupTrackQualities(int minBaseQ = 0) { const int rc = gnx_pileup_track_qualities(minBaseQ); if (rc) detail::raise(rc); }
inline void PileupAdd(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, const std::vector<std::vector<dna::Base>> &reads,
                      const std::vector<std::vector<uint8_t>> &quals, const std::vector<std::pair<int64_t, int64_t>> &windows, const std::vector<uint8_t> &strands,
                      const std::vector<std::vector<Cigar>> &routes, const std::vector<uint8_t> &use = {}) {
    detail::pile_add(scores, gapOpen, gapExtend, reads, &quals, windows, strands, routes, use);
}
inline std::vector<std::array<int32_t, 4>> PileupGetQual(int64_t first = 0, int64_t count = -1) {
    if (count < 0) count = PileupInfo().Len - first;
    std::vector<std::array<int32_t, 4>> rows((size_t)(count > 0 ? count : 0) + 1);
    const int rc = gnx_pileup_get_qual(first, count, rows[0].data());
    if (rc) detail::raise(rc);
    rows.pop_back();
    return rows;
}
inline std::vector<gnx_pile_genotype> PileupGenotypes(const GenoOpts &o = GenoOpts()) {
    const gnx_geno_opts go = {o.MinDepth, o.MinQual, o.PriorHet, o.PriorHom, {0, 0}};
    gnx_pile_genotype *recs = nullptr;
    int64_t n = 0;
    const int rc = gnx_pileup_genotypes(&go, &recs, &n);
    if (rc) detail::raise(rc);
    std::vector<gnx_pile_genotype> res(recs, recs + n);
    gnx_free(recs);
    return res;
}

// the alleles of the pile (gnx_pileup_track_alleles .. gnx_pileup_indel_calls): which deletion, which insertion
inline void PileupTrackAlleles(int64_t reserve = 0) { const int rc = gnx_pileup_track_alleles(reserve); if (rc) detail::raise(rc); }
// normalize: every allele is first moved to its leftmost placement against the reference inside the region (gnx_pileup_alleles_norm /
// gnx_pileup_indel_calls_norm); the pile and its log are not changed
inline std::vector<gnx_pile_allele> PileupAlleles(bool normalize = false) {
    gnx_pile_allele *res = nullptr;
    int64_t n = 0;
    const int rc = normalize ? gnx_pileup_alleles_norm(&res, &n) : gnx_pileup_alleles(&res, &n);
    if (rc) detail::raise(rc);
    std::vector<gnx_pile_allele> out(res, res + n);
    gnx_free(res);
    return out;
}
inline std::vector<gnx_pile_indel_call> PileupIndelCalls(const PileCallOpts &o = PileCallOpts(), bool normalize = false) {
    const gnx_pile_call_opts co = {o.MinDepth, o.MinAlt, o.FracNum, o.FracDen, o.BothStrands ? 1 : 0, 0};
    gnx_pile_indel_call *calls = nullptr;
    int64_t n = 0;
    const int rc = normalize ? gnx_pileup_indel_calls_norm(&co, &calls, &n) : gnx_pileup_indel_calls(&co, &calls, &n);
    if (rc) detail::raise(rc);
    std::vector<gnx_pile_indel_call> res(calls, calls + n);
    gnx_free(calls);
    return res;
}
// the inserted bases of a kind-2 allele's seq
inline std::vector<dna::Base> PileupAlleleBases(uint64_t seq) {
    std::vector<dna::Base> b;
    for (; seq; seq >>= 3) b.push_back((dna::Base)((seq & 7) - 1));
    return b;
}

inline void AffineGapLocalEngine(const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, std::vector<TargetQueryPair> &pairs) {
    std::vector<std::vector<dna::Base>> t, q;
    for (auto &p : pairs) { t.push_back(p.Target); q.push_back(p.Query); }
    std::vector<int64_t> sc; std::vector<std::vector<Cigar>> rt;
    AlignBatch(GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend, 10000, 10000, t, q, sc, rt);
    for (size_t k = 0; k < pairs.size(); k++) { pairs[k].Score = sc[k]; pairs[k].Cigar_ = std::move(rt[k]); }
}

// align.AffineGapChunk (align/affineGap_highMem.go:227-268), "next" row N1
inline std::pair<int64_t, std::vector<Cigar>> AffineGapChunk(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const ScoreMatrix &scores, int64_t gapOpen, int64_t gapExtend, int64_t chunkSize) {
    const gnx_params p = detail::params(GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend, 10000, 10000);
    const int64_t aoff[2] = {0, (int64_t)alpha.size()}, boff[2] = {0, (int64_t)beta.size()};
    int64_t score = 0, *off = nullptr;
    gnx_cigar *ops = nullptr;
    const int rc = gnx_affine_gap_chunk_batch(&p, chunkSize, 1, alpha.data(), aoff, beta.data(), boff, &score, &ops, &off);
    if (rc) detail::raise(rc);
    std::vector<Cigar> route((size_t)off[1]);
    for (int64_t k = 0; k < off[1]; k++) route[(size_t)k] = Cigar{ops[k].run_length, ops[k].op};
    gnx_free(ops); gnx_free(off);
    return {score, std::move(route)};
}

inline std::string PrintCigar(const std::vector<Cigar> &ops) { // align/view.go:26-33
    std::string s;
    for (const auto &c : ops) { s += std::to_string(c.RunLength); s += (c.Op == ColM ? 'M' : c.Op == ColI ? 'I' : c.Op == ColD ? 'D' : '?'); }
    return s;
}
inline std::string View(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const std::vector<Cigar> &ops) { // align/view.go:37-60
    const std::string a = dna::BasesToString(alpha), b = dna::BasesToString(beta);
    std::string one, two;
    size_t i = 0, j = 0;
    for (const auto &c : ops) {
        const size_t n = (size_t)c.RunLength;
        if (c.Op == ColM) { one += a.substr(i, n); two += b.substr(j, n); i += n; j += n; }
        else if (c.Op == ColI) { one += std::string(n, '-'); two += b.substr(j, n); j += n; }
        else if (c.Op == ColD) { one += a.substr(i, n); two += std::string(n, '-'); i += n; }
    }
    return one + "\n" + two + "\n";
}
} // namespace align
#endif

// ---- "next" row N2: the seed-extension DPs of the graph aligner (genomeGraph/search.go:234-321) -------------------------
namespace cigar {
struct Cigar { int64_t RunLength; uint8_t Op; }; // cigar.Cigar{RunLength int; Op byte}: 'M', 'I', 'D'
inline bool operator==(const Cigar &a, const Cigar &b) { return a.RunLength == b.RunLength && a.Op == b.Op; }
} // namespace cigar

namespace genomeGraph {
struct DynamicAln { int64_t score; std::vector<cigar::Cigar> route; int i, j; };

namespace detail {
inline DynamicAln extend(int side, const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const align::ScoreMatrix &scores, int64_t gapPen) {
    int64_t flat[25];
    for (int a = 0; a < 5; a++) for (int b = 0; b < 5; b++) flat[a * 5 + b] = scores[(size_t)a][(size_t)b];
    const int64_t aoff[2] = {0, (int64_t)alpha.size()}, boff[2] = {0, (int64_t)beta.size()};
    int64_t score = 0, ei = 0, ej = 0, *off = nullptr;
    gnx_cigar *ops = nullptr;
    const int rc = gnx_gsw_extend_batch(side, flat, gapPen, 1, alpha.data(), aoff, beta.data(), boff, &score, &ei, &ej, &ops, &off);
    if (rc) align::detail::raise(rc);
    DynamicAln out{score, {}, (int)ei, (int)ej};
    static const uint8_t letter[3] = {'M', 'I', 'D'};
    for (int64_t k = 0; k < off[1]; k++) out.route.push_back(cigar::Cigar{ops[k].run_length, letter[ops[k].op]});
    gnx_free(ops); gnx_free(off);
    return out;
}
} // namespace detail

// Route in traceback order, as the reference returns it for an empty incoming dynamicScore.route.
inline DynamicAln LeftDynamicAln(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const align::ScoreMatrix &scores, int64_t gapPen) {
    return detail::extend(GNX_GSW_LEFT, alpha, beta, scores, gapPen);
}
inline DynamicAln RightDynamicAln(const std::vector<dna::Base> &alpha, const std::vector<dna::Base> &beta, const align::ScoreMatrix &scores, int64_t gapPen) {
    return detail::extend(GNX_GSW_RIGHT, alpha, beta, scores, gapPen);
}
} // namespace genomeGraph
