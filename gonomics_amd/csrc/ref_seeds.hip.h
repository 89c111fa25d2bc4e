// ref_seeds.hip.h -- the k-mer index of the resident reference and seed-and-vote candidate windows for gnx_best_of_by_offset
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.20.
#pragma once
#include "gnx_common.hip.h"

namespace {
// ------------------------------------------------------------------------------------------------------
// Index (gnx_reference_index_build): positions p = 0, step, 2 step, ... with p + k <= len of the PACKED reference (KParams::b2 /
// bflag / brank / bexc: never the unpacked bytes); key = 2-bit code of ref[p .. p + k), first base most significant (dnaToNumber,
// genomeGraph/align.go:170); a k-mer that touches a base on the exception list (N, a byte >= 5) is skipped.  One thread per
// position flags it, an exclusive scan compacts (keys are formed again by the compacting kernel: no per-slot key array), one
// stable rocprim::radix_sort_pairs over 2 k bits orders by key with equal keys in ascending position.  Positions are 64-bit.
//
// Candidates (gnx_seed_candidates), per read and strand s (1: the reverse complement) and read position q:
//   stage 1  ref_seed_lookup_kernel   one thread per slot (read, s, q): the code of x[q .. q + k), binary search in the sorted
//                                     keys of its prefix (ref_index_dir_kernel's directory), (first, occ) per slot -- occ = 0 for a k-mer with an N, without entries or with more
//                                     than max_occ of them -- and the read's total in hits[read]
//   stage 2  ref_seed_vote_kernel     one wave per read: every entry's position t votes for (s, floor((t - q) / bin)) in an
//                                     open-addressing table (key claimed with a 32-bit compare-and-swap, count an atomic add) --
//                                     in LDS when 2 * hits fit VOTE_LDS_SLOTS, else in a slab of device memory of a power of two
//                                     >= 2 * hits slots --, then max_cand rounds of a wave-wide maximum over (votes, inverted
//                                     strand and bin), the winner removed each round
//   stage 3  ref_seed_windows_kernel  behind a scan of the candidate counts: the windows, compacted
// Votes commute and the order (votes descending, strand ascending, bin ascending) is total: the result does not depend on launch
// geometry, sub-batch cuts or execution order.
// ------------------------------------------------------------------------------------------------------
constexpr int VOTE_LDS_SLOTS = 1024; // 8 KB of LDS per one-wave workgroup (7 granules of 1280 B): 18 workgroups per CU, 4.5 waves per SIMD; serves reads of up to 512 hits

__host__ __device__ __forceinline__ int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int64_t i64max(int64_t a, int64_t b) { return a > b ? a : b; }
// true when ref[p .. p + k) holds nothing but A C G T (k <= 64: at most two 64-base blocks)
__device__ __forceinline__ bool ref_kmer_clean(const KParams &kp, int64_t p, int k) {
    for (int64_t blk = p >> 6; blk <= (p + k - 1) >> 6; blk++) {
        const unsigned long long f = kp.bflag[blk >> 6];
        const int bit = (int)(blk & 63);
        if (!((f >> bit) & 1ull)) continue;
        const int64_t e = (int64_t)kp.brank[blk >> 6] + __popcll(f & ((1ull << bit) - 1ull));
        const unsigned long long m = kp.bexc[2 * e] | kp.bexc[2 * e + 1];
        const int lo = (int)(i64max(p, blk << 6) - (blk << 6)), hi = (int)(i64min(p + k, (blk + 1) << 6) - (blk << 6)); // bits [lo, hi)
        const unsigned long long span = (hi - lo >= 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;
        if (m & span) return false;
    }
    return true;
}
__device__ __forceinline__ uint64_t ref_kmer_key(const unsigned *__restrict__ w2, int64_t p, int k) {
    uint64_t key = 0;
    unsigned w = w2[p >> 4];
    for (int i = 0; i < k; i++) {
        const int64_t x = p + i;
        if (i > 0 && (x & 15) == 0) w = w2[x >> 4];
        key = (key << 2) | (uint64_t)((w >> (2 * ((int)x & 15))) & 3u);
    }
    return key;
}
// slots [s0, s0 + n) of the index: flag[x - s0] = 1 when position x * step has a k-mer
__global__ __launch_bounds__(256) void ref_index_flag_kernel(KParams kp, int64_t s0, int64_t n, int seed_len, int seed_step, int64_t *__restrict__ flag) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    flag[x] = ref_kmer_clean(kp, (s0 + x) * seed_step, seed_len) ? 1 : 0;
}
// off = exclusive scan of flag (carried over the chunks before): the flagged slots' (key, position) at off[x]
__global__ __launch_bounds__(256) void ref_index_emit_kernel(KParams kp, int64_t s0, int64_t n, int seed_len, int seed_step, const int64_t *__restrict__ flag,
                                                             const int64_t *__restrict__ off, uint64_t *__restrict__ keys, uint64_t *__restrict__ pos) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n || !flag[x]) return;
    const int64_t p = (s0 + x) * seed_step;
    keys[off[x]] = ref_kmer_key(kp.b2, p, seed_len);
    pos[off[x]] = (uint64_t)p;
}

// dir[x] = the first index entry whose key has a prefix >= x (the top bits of the 2 k key bits; dir[n_dir] = n): a lookup searches
// the handful of entries of its prefix instead of the whole index
__global__ __launch_bounds__(256) void ref_index_dir_kernel(const uint64_t *__restrict__ keys, int64_t n, int shift, int64_t n_dir, int64_t *__restrict__ dir) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > n_dir) return;
    int64_t l = n;
    if (x < n_dir) {
        const uint64_t key = (uint64_t)x << shift;
        int64_t h = n;
        l = 0;
        while (l < h) { const int64_t mid = (l + h) >> 1; if (keys[mid] < key) l = mid + 1; else h = mid; }
    }
    dir[x] = l;
}

struct SeedVoteArgs {
    const uint64_t *keys, *pos; int64_t n_index; // the index
    const int64_t *dir; int dir_shift;           // ... and its directory by key prefix (key >> dir_shift)
    const uint8_t *reads; const int64_t *read_off, *slot_off; // reads of this piece; slot_off[r] = 2 * k-mer positions of the reads before r
    int64_t *first; int *occ; unsigned long long *hits;       // per slot; per read
    unsigned long long *stage; int64_t *cnt;                  // per read: max_cand composite keys (votes << 32 | ~table key); candidates kept
    int64_t ref_len;
    int seed_len, max_occ, bin, bin_shift, pad, max_cand, min_votes; // bin_shift >= 0: bin == 1 << bin_shift
};
// bins are counted from the lowest one a read of n bases can vote for: diagonal d >= -(n - k), so d + vote_bias(n) * bin >= 0
__device__ __forceinline__ int64_t vote_bias(int64_t n, int k, int bin) { return (n - k + bin - 1) / bin; }

__global__ __launch_bounds__(256) void ref_seed_lookup_kernel(SeedVoteArgs a, int n_reads, int64_t n_slots) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_slots) return;
    int lo = 0, hi = n_reads - 1; // read of slot x: the last one with slot_off <= x
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.slot_off[mid] <= x) lo = mid; else hi = mid - 1; }
    const int r = lo;
    const int64_t n = a.read_off[r + 1] - a.read_off[r], npos = n - a.seed_len + 1, rel = x - a.slot_off[r];
    const int s = rel >= npos ? 1 : 0;
    const int64_t q = rel - (s ? npos : 0);
    const uint8_t *rd = a.reads + a.read_off[r];
    uint64_t key = 0;
    bool ok = true;
    for (int i = 0; i < a.seed_len; i++) { // strand 1: x[j] = complement of read[n - 1 - j] (dna.ReverseComplement)
        const uint8_t v = s ? rd[n - 1 - q - i] : rd[q + i];
        if (v >= 4) ok = false;
        key = (key << 2) | (uint64_t)((s ? 3 - v : v) & 3);
    }
    int64_t first = 0, cnt = 0;
    if (ok) {
        const uint64_t pre = key >> a.dir_shift;
        int64_t l = a.dir[pre];
        const int64_t end = a.dir[pre + 1]; // entries of this prefix: [l, end)
        int64_t h = end;
        while (l < h) { const int64_t mid = (l + h) >> 1; if (a.keys[mid] < key) l = mid + 1; else h = mid; }
        first = l;
        if (l < end && a.keys[l] == key) { // the run of equal keys is short as a rule: gallop, then bisect (l: equal; h: not equal, or the end)
            int64_t st = 1;
            h = l + 1;
            while (h < end && a.keys[h] == key) { l = h; st <<= 1; h = i64min(end, l + st); }
            while (h - l > 1) { const int64_t mid = (l + h) >> 1; if (a.keys[mid] == key) l = mid; else h = mid; }
            cnt = h - first;
        }
        if (cnt > a.max_occ) cnt = 0;
    }
    a.first[x] = first;
    a.occ[x] = (int)cnt;
    if (cnt) atomicAdd(&a.hits[r], (unsigned long long)cnt);
}

struct VoteItem { int32_t read, lg; int64_t slab_off; }; // slab form: 2^lg slots of (key + 1, votes) at slab[2 * slab_off ..)
template <bool LDS> __device__ __forceinline__ unsigned vt_load(const unsigned *p) { return LDS ? *p : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <bool LDS> __device__ __forceinline__ void vt_store(unsigned *p, unsigned v) { if (LDS) *p = v; else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}
// One wave per read.  Table slot: tk = key + 1 (0: empty), key = strand << 30 | (bin + bias); tc = votes.  The slab form is zeroed by the host.
template <bool LDS>
__global__ __launch_bounds__(64) void ref_seed_vote_kernel(SeedVoteArgs a, const VoteItem *__restrict__ items, unsigned *__restrict__ slab) {
    __shared__ unsigned lds_tab[LDS ? 2 * VOTE_LDS_SLOTS : 2];
    const VoteItem it = items[blockIdx.x];
    const int lane = (int)threadIdx.x, r = it.read, lg = LDS ? 10 : it.lg;
    static_assert(VOTE_LDS_SLOTS == 1 << 10, "lg of the LDS table");
    const unsigned S = 1u << lg;
    unsigned *tk = LDS ? lds_tab : slab + 2 * it.slab_off, *tc = tk + S;
    if (LDS) { for (unsigned i = (unsigned)lane; i < 2 * S; i += 64) tk[i] = 0u; }
    __syncthreads();
    const int64_t n = a.read_off[r + 1] - a.read_off[r], npos = n - a.seed_len + 1, base = a.slot_off[r];
    const int64_t shift = vote_bias(n, a.seed_len, a.bin) * a.bin;
    for (int64_t i = lane; i < 2 * npos; i += 64) {
        const int cnt = a.occ[base + i];
        if (!cnt) continue;
        const int64_t first = a.first[base + i];
        const unsigned s = i >= npos ? 1u : 0u;
        const int64_t q = i - (s ? npos : 0);
        for (int h = 0; h < cnt; h++) {
            const uint64_t y = (uint64_t)((int64_t)a.pos[first + h] - q + shift); // >= 0: floor division is plain division
            const unsigned key1 = ((s << 30) | (unsigned)(a.bin_shift >= 0 ? y >> a.bin_shift : y / (uint64_t)a.bin)) + 1u;
            unsigned at = (key1 * 2654435761u) >> (32 - lg);
            for (;;) { // at most 2^lg / 2 distinct keys: the probe ends
                const unsigned prev = atomicCAS(&tk[at], 0u, key1);
                if (prev == 0u || prev == key1) { atomicAdd(&tc[at], 1u); break; }
                at = (at + 1u) & (S - 1u);
            }
        }
    }
    __syncthreads();
    int kept = 0;
    for (; kept < a.max_cand; kept++) {
        unsigned long long best = 0;
        unsigned bi = 0;
        for (unsigned i = (unsigned)lane; i < S; i += 64) {
            const unsigned v = vt_load<LDS>(&tc[i]);
            if (!v) continue;
            const unsigned long long comp = ((unsigned long long)v << 32) | (unsigned long long)(0xffffffffu - (vt_load<LDS>(&tk[i]) - 1u));
            if (comp > best) { best = comp; bi = i; }
        }
        const unsigned long long top = wave_max_u64(best);
        if ((long long)(top >> 32) < (long long)a.min_votes) break;
        if (best == top) vt_store<LDS>(&tc[bi], 0u); // keys are distinct: exactly one lane
        if (lane == 0) a.stage[(int64_t)r * a.max_cand + kept] = top;
        __syncthreads();
    }
    if (lane == 0) a.cnt[r] = kept;
}
// one thread per (read, j < max_cand): candidate j of read r at off[r] + j
__global__ __launch_bounds__(256) void ref_seed_windows_kernel(SeedVoteArgs a, int64_t n_reads, const int64_t *__restrict__ off,
                                                               int64_t *__restrict__ c_start, int64_t *__restrict__ c_len, uint8_t *__restrict__ c_strand, int32_t *__restrict__ c_votes) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_reads * a.max_cand) return;
    const int64_t r = x / a.max_cand, j = x - r * a.max_cand;
    if (j >= a.cnt[r]) return;
    const unsigned long long comp = a.stage[x];
    const unsigned key = 0xffffffffu - (unsigned)comp;
    const int64_t n = a.read_off[r + 1] - a.read_off[r];
    const int64_t b = (int64_t)(key & 0x3fffffffu) - vote_bias(n, a.seed_len, a.bin);
    const int64_t start = i64min(i64max(b * a.bin - a.pad, 0), a.ref_len), end = i64min(i64max((b + 1) * a.bin + n + a.pad, 0), a.ref_len);
    const int64_t o = off[r] + j;
    c_start[o] = start; c_len[o] = end - start; c_strand[o] = (uint8_t)(key >> 30); c_votes[o] = (int32_t)(comp >> 32);
}

} // namespace
