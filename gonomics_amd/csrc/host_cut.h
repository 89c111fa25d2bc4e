// host_cut.h -- how the host flows cut a batch into sub-batches (gnx_host.hip.h), plain C++: no HIP header needed.
// Shared by run_host_job, run_best_of, run_summarize and run_md, and by tests/cpp/host_cut_test.cpp on the CPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>

// The sub-batch limit in pairs: 131072 unless GNX_HOST_SUB (`env` = its value, or null) says otherwise; at least 8, whole waves.
inline int64_t gnx_host_sub(const char *env) {
    if (!env) return 131072;
    const int64_t v = atoll(env);
    return ((v > 8 ? v : 8) + 7) & ~(int64_t)7;
}

// n pairs in sub-batches of at most `sub` (> 0): equal sizes (the fast path re-uses its plans), whole waves; 0 for n == 0.  A caller
// steps through [0, n) by this size and clips the last one: rounding up can save a sub-batch, so nothing may index past n.
inline int64_t sub_batch_size(int64_t n, int64_t sub) {
    if (n <= 0) return 0;
    const int64_t K0 = (n + sub - 1) / sub;
    return (((n + K0 - 1) / K0) + 7) & ~(int64_t)7;
}
