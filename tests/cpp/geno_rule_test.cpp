// geno_rule() of gonomics_amd/csrc/geno_rule.h on the CPU: the function geno_call_kernel calls, compiled by a plain C++ compiler.
// Reads one position per line from stdin -- fwd[4] rev[4] qsum[4] c min_depth min_qual prior_het prior_hom, 17 integers -- and prints its
// record, "gt alt pl0 pl1 pl2 gq qual depth ref_count alt_count alt_fwd", or "none".  tests/test_pile_qual_cpu.py compares the lines with
// the restatement (tests/pyref_pile_qual.py).
#include <cstdio>

#include "geno_rule.h"

int main() {
    long long v[17];
    for (;;) {
        int got = 0;
        while (got < 17 && std::scanf("%lld", &v[got]) == 1) got++;
        if (got == 0) return 0;
        if (got != 17) { std::fprintf(stderr, "a line of %d integers\n", got); return 1; }
        int32_t fwd[4], rev[4], qsum[4];
        for (int a = 0; a < 4; a++) { fwd[a] = (int32_t)v[a]; rev[a] = (int32_t)v[4 + a]; qsum[a] = (int32_t)v[8 + a]; }
        const GenoOpts o = {(int32_t)v[13], (int32_t)v[14], (int32_t)v[15], (int32_t)v[16]};
        GenoRec r;
        if (geno_rule(fwd, rev, qsum, (int)v[12], o, r))
            std::printf("%d %d %d %d %d %d %d %d %d %d %d\n", r.gt, r.alt, r.pl[0], r.pl[1], r.pl[2], r.gq, r.qual, r.depth, r.ref_count, r.alt_count, r.alt_fwd);
        else std::printf("none\n");
    }
}
