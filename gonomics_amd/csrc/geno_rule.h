// geno_rule.h -- the diploid SNP genotype rule of gnx_pileup_genotypes at ONE position (contract: gnx_align.h), plain
// C++: no HIP header needed.  Shared by geno_call_kernel (pile_qual.hip.h) and by tests/cpp/geno_rule_test.cpp on the CPU.
//
// Integer only, in centi-Phred (1/100 of a Phred unit).  With n[a] the read bases of letter a over the position (both strands), Q[a]
// the sum of their qualities and c the reference code:
//   E[a] = 100 * Q[a] + 477 * n[a]     what it costs to explain all a bases as errors (477 = round(1000 * log10 3): a miscall lands on
//                                      one of three letters; the -10 log10(1 - e) term of the correct bases is dropped)
//   b    = the a != c with the largest E[a], ties to the smaller index
//   L[0] = E[b]                                  ref / ref
//   L[1] = 301 * (n[c] + n[b]) + prior_het       ref / alt   (301 = round(1000 * log10 2))
//   L[2] = E[c] + prior_hom                      alt / alt
// The bases of the other two letters cost every genotype the same and cancel.  g = argmin L (ties to the smaller index),
// pl[k] = L[k] - L[g], gq = the smallest pl[k] with k != g, qual = max(0, L[0] - min(L[1], L[2])); pl, gq and qual saturate at 2^31 - 1.
// A record is emitted iff depth >= min_depth, g != 0 and qual >= min_qual; a reference N (c >= 4) is silent.
// Everything is summed in 64 bits: counts and quality sums up to 2^31 - 1 per strand cannot overflow (E < 2^41).  depth, ref_count and
// alt_count saturate at 2^31 - 1 as well -- no pile reaches that (its reads are bounded), the rule is total all the same.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GNX_GENO_HD __host__ __device__
#else
#define GNX_GENO_HD
#endif

struct GenoOpts { int32_t min_depth, min_qual, prior_het, prior_hom; };
struct GenoRec {
    int32_t pl[3], gq, qual, depth, ref_count, alt_count, alt_fwd;
    int32_t gt, alt; // gt 1 (ref / alt) or 2 (alt / alt); alt: the base code
};

GNX_GENO_HD inline int32_t geno_sat(int64_t v) { return v > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)v; }

// fwd[a], rev[a]: the strand counts of A C G T; qsum[a]: the quality sums, both strands; c: the reference code.  true: r is the record.
GNX_GENO_HD inline bool geno_rule(const int32_t fwd[4], const int32_t rev[4], const int32_t qsum[4], int c, const GenoOpts &o, GenoRec &r) {
    if (c < 0 || c >= 4) return false;
    int64_t n[4], E[4], depth = 0;
    for (int a = 0; a < 4; a++) {
        n[a] = (int64_t)fwd[a] + rev[a];
        E[a] = 100 * (int64_t)qsum[a] + 477 * n[a];
        depth += n[a];
    }
    // (b and c pick their values in unrolled loops, not by indexing with a run-time value: the arrays stay in registers on the device)
    int b = -1;
    int64_t nb = 0, Eb = 0, nc = 0, Ec = 0;
    int32_t fb = 0;
    for (int a = 0; a < 4; a++) {
        if (a == c) { nc = n[a]; Ec = E[a]; }
        else if (b < 0 || E[a] > Eb) { b = a; nb = n[a]; Eb = E[a]; fb = fwd[a]; }
    }
    const int64_t L0 = Eb, L1 = 301 * (nc + nb) + o.prior_het, L2 = Ec + o.prior_hom;
    int g = 0;
    int64_t best = L0;
    if (L1 < best) { best = L1; g = 1; }
    if (L2 < best) { best = L2; g = 2; }
    const int64_t p0 = L0 - best, p1 = L1 - best, p2 = L2 - best;
    const int64_t gq = g == 0 ? (p1 < p2 ? p1 : p2) : g == 1 ? (p0 < p2 ? p0 : p2) : (p0 < p1 ? p0 : p1);
    const int64_t m12 = L1 < L2 ? L1 : L2;
    const int64_t qual = L0 - m12 > 0 ? L0 - m12 : 0;
    if (depth < o.min_depth || g == 0 || qual < o.min_qual) return false;
    r.pl[0] = geno_sat(p0); r.pl[1] = geno_sat(p1); r.pl[2] = geno_sat(p2);
    r.gq = geno_sat(gq); r.qual = geno_sat(qual);
    r.depth = geno_sat(depth); r.ref_count = geno_sat(nc); r.alt_count = geno_sat(nb); r.alt_fwd = fb;
    r.gt = g; r.alt = b;
    return true;
}
