// The sub-batch cut of the host flows (gonomics_amd/csrc/host_cut.h) on the CPU: whole waves, nothing past n, no empty sub-batch,
// and the same numbers as the three lines the flows used to spell out each for itself.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "host_cut.h"

static int fails = 0;
#define EXPECT(cond, ...)                                                                 \
    do {                                                                                  \
        if (!(cond)) { fails++; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

int main() {
    const int64_t subs[] = {8, 12, 64, 100, 131072};
    const int64_t ns[] = {0, 1, 7, 8, 9, 1000, 1001, 131072, 131073, 1000000};
    for (int64_t sub_in : subs) {
        char text[32];
        snprintf(text, sizeof(text), "%lld", (long long)sub_in);
        // the restatement of the parsing: int64_t sub = 131072; if (e) sub = (max(atoll(e), 8) + 7) & ~7
        const int64_t sub_ref = (std::max<int64_t>(atoll(text), 8) + 7) & ~(int64_t)7;
        const int64_t sub = gnx_host_sub(text);
        EXPECT(sub == sub_ref, "sub %lld: %lld != %lld", (long long)sub_in, (long long)sub, (long long)sub_ref);
        for (int64_t n : ns) {
            const int64_t size = sub_batch_size(n, sub);
            const int64_t K = n > 0 ? (n + size - 1) / size : 0;
            EXPECT(size % 8 == 0, "sub %lld n %lld: size %lld", (long long)sub_in, (long long)n, (long long)size);
            EXPECT(K * size >= n, "sub %lld n %lld: K %lld size %lld", (long long)sub_in, (long long)n, (long long)K, (long long)size);
            if (n > 0) {
                EXPECT((K - 1) * size < n, "sub %lld n %lld: K %lld size %lld", (long long)sub_in, (long long)n, (long long)K, (long long)size);
                EXPECT(size <= ((n + 7) & ~(int64_t)7) && size <= sub, "sub %lld n %lld: size %lld", (long long)sub_in, (long long)n, (long long)size);
                // the restatement of the cut
                const int64_t K0 = (n + sub_ref - 1) / sub_ref;
                const int64_t size_ref = (((n + K0 - 1) / K0) + 7) & ~(int64_t)7;
                const int64_t K_ref = (n + size_ref - 1) / size_ref;
                EXPECT(size == size_ref && K == K_ref, "sub %lld n %lld: %lld x %lld != %lld x %lld", (long long)sub_in, (long long)n, (long long)K, (long long)size,
                       (long long)K_ref, (long long)size_ref);
            } else
                EXPECT(size == 0, "n 0: size %lld", (long long)size);
        }
    }
    // the parsing's edges: unset, too small, not a multiple of 8, not a number
    EXPECT(gnx_host_sub(nullptr) == 131072, "unset");
    EXPECT(gnx_host_sub("1") == 8 && gnx_host_sub("0") == 8 && gnx_host_sub("-5") == 8 && gnx_host_sub("x") == 8, "small values");
    EXPECT(gnx_host_sub("12") == 16 && gnx_host_sub("200") == 200 && gnx_host_sub("1000000") == 1000000, "rounding");
    // sub = 12 once gave 84 sub-batches of 16 for n = 1000, the last ones past n
    EXPECT(sub_batch_size(1000, gnx_host_sub("12")) == 16 && (1000 + 15) / 16 == 63, "sub 12, n 1000");
    if (fails) { printf("%d failure(s)\n", fails); return 1; }
    printf("host_cut ok\n");
    return 0;
}
