// aux_kernels.hip.h -- N1 score matrices, run scaling, exclusive scan of the run counts, window unpacking, the best-of-K helpers, the pair selection
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md section 4.
#pragma once
#include "gnx_common.hip.h"

namespace {
// ------------------------------------------------------------------------------------------------------
// N1: per-cell score matrices for the chunk / multiple-alignment variants, one thread per (chunk) cell, written
// column-major as 4*score (+ bias4, see the kernel).  A "group" is an alignment block: nseq sequences of len bases, sequence-major.
//   pairwise (AffineGapChunk):      cell = sum_k scores[a[i*c+k]][b[j*c+k]]                       (ungapped.go:7-13)
//   groups (multipleAffineGap*):    cell = sum_k scoreColumnMatch(column i*c+k, column j*c+k)     (multiAlign.go:82-110)
//     scoreColumnMatch = (sum over sequence pairs, lower case folded, gap columns skipped) / count, Go integer division
// ------------------------------------------------------------------------------------------------------
struct GroupDesc { int64_t off; int32_t nseq; int32_t len; };
struct ScorePair { int64_t a_off, b_off; int32_t a_nseq, b_nseq, a_len, b_len; int32_t nc, mc; int64_t s_off, s_pitch; int64_t pa_off, pb_off; }; // pa_off / pb_off: column profiles of the two groups (score_profiles_kernel), in entries

// the SWP store of four rows of a column (see score_matrix_kernel): rows >= nc are not written (the next column's padding follows),
// the thread of row 0 also writes the column's padding
__device__ __forceinline__ void sweep_store4(short *__restrict__ dst, const int (&out)[4], int i0, int nc) {
#pragma unroll
    for (int r = 0; r < 4; r++) if (i0 + r < nc) dst[r] = (short)(out[r] >> 2);
    if (i0 == 0) { const int pad = (10 - nc % 10) % 10; for (int k = 1; k <= pad; k++) dst[-k] = (short)-32768; }
}

// S16: every 4*score fits int16 (host check: 4 * chunk * max|score| <= 32767) -- the matrix is stored as int16, which halves the
// HBM traffic of the SCORED fill (it reads one entry per cell and is bandwidth-bound with 4-byte entries)
// SWP: the layout of the score-only sweep (n1_sweep.hip.h): plain int16 entries s - 2e (bias4 = -8e), a column = [pad entries of
// -32768][rows 0 .. nc - 1] with pad = (10 - nc % 10) % 10; s_off is the entry of row 0 of column 0 and s_pitch = nc + pad (no slack)
template <bool S16, bool SWP = false>
__global__ __launch_bounds__(256) void score_matrix_kernel(const ScorePair *__restrict__ sp, const uint8_t *__restrict__ bases, KParams kp, int chunk,
                                                           int groups, int bias4, int *__restrict__ smat, int *__restrict__ err) {
    // bias4 = -2 * 4 * gapExtend * chunk when the fill runs on rebased keys (fill_affine_kernel, HFORM), else 0
    // block = 64 x 4 threads: x runs over GROUPS OF FOUR rows i (the fast index of the column-major matrix: one 8- / 16-byte store per
    // thread and column instead of four 2- / 4-byte ones), y over 4 columns j; grid.x strides over the columns, grid.y = pair.
    // No per-cell division; the 5 x 5 table sits in LDS.  (Rows nc .. of the last group of four lie inside the pitch and are never read.)
    __shared__ int sc[25];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if (tid < 25) sc[tid] = kp.sc4[tid] / 4;
    __syncthreads();
    const ScorePair q = sp[blockIdx.y];
    for (int j = blockIdx.x * 4 + threadIdx.y; j < q.mc; j += gridDim.x * 4) {
        for (int i0 = threadIdx.x * 4; i0 < q.nc; i0 += 256) {
            int out[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + r;
                int64_t total = 0;
                for (int k = 0; i < q.nc && k < chunk; k++) {
                    const int64_t ac = (int64_t)i * chunk + k, bc = (int64_t)j * chunk + k;
                    if (!groups) {
                        const int a = bases[q.a_off + ac], b = bases[q.b_off + bc];
                        if (a >= 5 || b >= 5) { atomicOr(err, 1); continue; }
                        total += sc[a * 5 + b];
                    } else {
                        int64_t sum = 0, count = 0;
                        for (int x = 0; x < q.a_nseq; x++) {
                            int a = bases[q.a_off + (int64_t)x * q.a_len + ac];
                            if (a >= 5 && a <= 9) a -= 5;
                            for (int y = 0; y < q.b_nseq; y++) {
                                int b = bases[q.b_off + (int64_t)y * q.b_len + bc];
                                if (b >= 5 && b <= 9) b -= 5;
                                if (a != 10 && b != 10) {
                                    if (a >= 5 || b >= 5) { atomicOr(err, 1); continue; }
                                    sum += sc[a * 5 + b];
                                    count++;
                                }
                            }
                        }
                        if (count == 0) { atomicOr(err, 16); continue; } // Go: integer divide by zero
                        total += sum / count;
                    }
                }
                out[r] = (int)(4 * total) + bias4;
            }
            const int64_t at = q.s_off + (int64_t)j * q.s_pitch + i0; // multiple of 4: s_off and s_pitch are multiples of 160
            if constexpr (SWP) sweep_store4(reinterpret_cast<short *>(smat) + at, out, i0, q.nc);
            else if (S16) *reinterpret_cast<uint2 *>(reinterpret_cast<short *>(smat) + at) = make_uint2((unsigned)(out[0] & 0xffff) | ((unsigned)out[1] << 16), (unsigned)(out[2] & 0xffff) | ((unsigned)out[3] << 16));
            else *reinterpret_cast<int4 *>(smat + at) = make_int4(out[0], out[1], out[2], out[3]);
        }
    }
}

// The pairwise case (AffineGapChunk: cell (i, j) = sum over the chunk's positions of scores[alpha][beta]) for chunk sizes 1 .. 4, which is
// what the callers use: a thread keeps the bases of its four rows in registers and walks the columns (the general kernel above
// re-reads them, with 64-bit index arithmetic, for every cell: 6 ms for 4096 pairs of 160 x 3000 chunks, more than the fill).
// block = 64 x 4 threads: x = groups of four rows, y = 4 columns; a block walks the columns blockIdx.x * 4 + y, + 4 * gridDim.x, ...
template <bool S16, int CH, bool SWP = false>
__global__ __launch_bounds__(256) void score_matrix_pairs_kernel(const ScorePair *__restrict__ sp, const uint8_t *__restrict__ bases, KParams kp, int bias4,
                                                                 int *__restrict__ smat, int *__restrict__ err) {
    __shared__ int sc[32];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if (tid < 25) sc[tid] = kp.sc4[tid]; // 4 * score
    __syncthreads();
    const ScorePair q = sp[blockIdx.y];
    const uint8_t *ap = bases + q.a_off, *bq = bases + q.b_off;
    int bad = 0;
    for (int i0 = threadIdx.x * 4; i0 < q.nc; i0 += 256) {
        int a5[4][CH];
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int k = 0; k < CH; k++) {
                int a = (i0 + r < q.nc) ? ap[(i0 + r) * CH + k] : 0; // (rows nc .. of the last group of four lie inside the pitch and are never read)
                if (a >= 5) { bad = 1; a = 0; }
                a5[r][k] = a * 5;
            }
        }
        for (int j = blockIdx.x * 4 + threadIdx.y; j < q.mc; j += gridDim.x * 4) {
            int out[4] = {bias4, bias4, bias4, bias4};
#pragma unroll
            for (int k = 0; k < CH; k++) {
                int b = bq[j * CH + k];
                if (b >= 5) { bad = 1; b = 0; }
#pragma unroll
                for (int r = 0; r < 4; r++) out[r] += sc[a5[r][k] + b];
            }
            const int64_t at = q.s_off + (int64_t)j * q.s_pitch + i0;
            if constexpr (SWP) sweep_store4(reinterpret_cast<short *>(smat) + at, out, i0, q.nc);
            else if (S16) *reinterpret_cast<uint2 *>(reinterpret_cast<short *>(smat) + at) = make_uint2((unsigned)(out[0] & 0xffff) | ((unsigned)out[1] << 16), (unsigned)(out[2] & 0xffff) | ((unsigned)out[3] << 16));
            else *reinterpret_cast<int4 *>(smat + at) = make_int4(out[0], out[1], out[2], out[3]);
        }
    }
    if (bad) atomicOr(err, 1);
}

// ---- groups, round 5: column profiles instead of a loop over all sequence pairs per cell ---------------------------------------------
// scoreColumnMatch(u, v) = (sum over members x of A and y of B, gaps skipped, lower case folded, of scores[a_x(u)][b_y(v)]) / count
//                        = (sum_a cntA[u][a] * wB[v][a]) / (nA(u) * nB(v)),   wB[v][a] = sum_b scores[a][b] * cntB[v][b]
// with cnt = how many members show base a in the column and n = how many show a base at all: five multiply-adds and one truncating
// division per column pair whatever the group sizes (and no division at all while both groups are single sequences: the first round of
// AllSeqAffineChunk).  The old kernel above walked every member pair of every cell with 64-bit arithmetic: 25 ms for the 28 pairs of 10 000 x
// 10 000 chunk cells of a cmd/faChunkAlign round, three times the DP itself.
struct ColProfA { short cnt[5]; short n; short bad; short pad; };          // 16 B per column of group A
struct ColProfB { int w[5]; int n; int bad; int pad; };                     // 32 B per column of group B
__global__ __launch_bounds__(256) void score_profiles_kernel(const ScorePair *__restrict__ sp, const uint8_t *__restrict__ bases, KParams kp,
                                                            ColProfA *__restrict__ pa, ColProfB *__restrict__ pb) {
    __shared__ int sc[25];
    if (threadIdx.x < 25) sc[threadIdx.x] = kp.sc4[threadIdx.x] / 4;
    __syncthreads();
    const ScorePair q = sp[blockIdx.y];
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < (int64_t)q.a_len + q.b_len; x += (int64_t)gridDim.x * blockDim.x) {
        const bool isb = x >= q.a_len;
        const int col = (int)(isb ? x - q.a_len : x), nseq = isb ? q.b_nseq : q.a_nseq, len = isb ? q.b_len : q.a_len;
        const uint8_t *src = bases + (isb ? q.b_off : q.a_off) + col;
        int cnt[5] = {0, 0, 0, 0, 0}, bad = 0;
        for (int m = 0; m < nseq; m++) {
            int a = src[(int64_t)m * len];
            if (a >= 5 && a <= 9) a -= 5; // lower case -> upper case (multiAlign.go:87-94)
            if (a == 10) continue;        // dna.Gap
            if (a > 10) { bad = 1; continue; }
#pragma unroll
            for (int z = 0; z < 5; z++) cnt[z] += (a == z);
        }
        const int n = cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4];
        if (!isb) {
            ColProfA o;
#pragma unroll
            for (int z = 0; z < 5; z++) o.cnt[z] = (short)cnt[z];
            o.n = (short)n; o.bad = (short)bad; o.pad = 0;
            pa[q.pa_off + col] = o;
        } else {
            ColProfB o;
#pragma unroll
            for (int a = 0; a < 5; a++) { int w = 0; for (int b = 0; b < 5; b++) w += sc[a * 5 + b] * cnt[b]; o.w[a] = w; }
            o.n = n; o.bad = bad; o.pad = 0;
            pb[q.pb_off + col] = o;
        }
    }
}
// block = 64 x 4 threads: x = groups of four chunk rows (their column profiles stay in registers), y = 4 chunk columns; see score_matrix_pairs_kernel
template <bool S16, int CH, bool SWP = false>
__global__ __launch_bounds__(256) void score_matrix_groups_kernel(const ScorePair *__restrict__ sp, KParams kp, int bias4, const ColProfA *__restrict__ pa,
                                                                  const ColProfB *__restrict__ pb, int *__restrict__ smat, int *__restrict__ err) {
    const ScorePair q = sp[blockIdx.y];
    const bool single = q.a_nseq == 1 && q.b_nseq == 1; // every count is 0 or 1: no division
    int flags = 0;
    for (int i0 = threadIdx.x * 4; i0 < q.nc; i0 += 256) {
        short ca[4][CH][5];
        int na[4][CH];
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int k = 0; k < CH; k++) {
                ColProfA o;
                if (i0 + r < q.nc) o = pa[q.pa_off + (int64_t)(i0 + r) * CH + k];
                else { for (int z = 0; z < 5; z++) o.cnt[z] = 0; o.n = 1; o.bad = 0; } // (rows nc .. of the last group of four lie inside the pitch and are never read)
#pragma unroll
                for (int z = 0; z < 5; z++) ca[r][k][z] = o.cnt[z];
                na[r][k] = o.n;
                flags |= o.bad ? 1 : 0;
            }
        }
        for (int j = blockIdx.x * 4 + threadIdx.y; j < q.mc; j += gridDim.x * 4) {
            int out[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < CH; k++) {
                const ColProfB o = pb[q.pb_off + (int64_t)j * CH + k];
                flags |= o.bad ? 1 : 0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    int sum = 0;
#pragma unroll
                    for (int z = 0; z < 5; z++) sum += (int)ca[r][k][z] * o.w[z];
                    const int count = na[r][k] * o.n;
                    if (count == 0) { if (i0 + r < q.nc) flags |= 16; continue; } // Go: integer divide by zero (multiAlign.go:101)
                    out[r] += single ? sum : sum / count;                     // Go's truncating division
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) out[r] = 4 * out[r] + bias4;
            const int64_t at = q.s_off + (int64_t)j * q.s_pitch + i0;
            if constexpr (SWP) sweep_store4(reinterpret_cast<short *>(smat) + at, out, i0, q.nc);
            else if (S16) *reinterpret_cast<uint2 *>(reinterpret_cast<short *>(smat) + at) = make_uint2((unsigned)(out[0] & 0xffff) | ((unsigned)out[1] << 16), (unsigned)(out[2] & 0xffff) | ((unsigned)out[3] << 16));
            else *reinterpret_cast<int4 *>(smat + at) = make_int4(out[0], out[1], out[2], out[3]);
        }
    }
    if (flags) atomicOr(err, flags);
}

__global__ __launch_bounds__(256) void scale_runs_kernel(gnx_cigar *__restrict__ ops, int64_t total, int64_t factor) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < total) ops[x].run_length *= factor; // expandCigarRunLength, affineGap_highMem.go:91-95
}

// exclusive scan of nops[0..n) + carry[0] -> off[0..n], off[n]; carry[0] = off[n] afterwards.  One block.
__global__ __launch_bounds__(1024) void scan_kernel(const int64_t *__restrict__ nops, int n, int64_t *__restrict__ off, int64_t *__restrict__ carry) {
    // exclusive scan of the run counts, 1024 elements per round: wave-level scans by __shfl_up, then the 16 wave totals
    // (a one-pass version with a contiguous slice per thread measured slower: 227 us vs 139 us per 100 k elements)
    __shared__ int64_t wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base = carry[0];
    for (int start = 0; start < n; start += 1024) {
        const int idx = start + threadIdx.x;
        const int64_t v = idx < n ? nops[idx] : 0;
        int64_t sum = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int64_t t = __shfl_up(sum, d, 64); if (lane >= d) sum += t; }
        if (lane == 63) wsum[wave] = sum;
        __syncthreads();
        if (wave == 0) {
            int64_t t = lane < 16 ? wsum[lane] : 0;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { const int64_t u = __shfl_up(t, d, 64); if (lane >= d) t += u; }
            if (lane < 16) wsum[lane] = t;
        }
        __syncthreads();
        if (idx < n) off[idx] = base + (wave > 0 ? wsum[wave - 1] : 0) + sum - v;
        base += wsum[15];
        __syncthreads();
    }
    if (threadIdx.x == 0) { off[n] = base; carry[0] = base; }
}

// Large inputs: three launches instead of one 1024-thread block walking the whole array (139 us per 100 k elements):
// per-block sums -> scan_kernel over the sums (it adds and updates the carry) -> per-block scans on top of their offsets.
__global__ __launch_bounds__(1024) void scan_sums_kernel(const int64_t *__restrict__ nops, int n, int64_t *__restrict__ sums) {
    __shared__ int64_t wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x * 1024 + threadIdx.x;
    int64_t v = idx < n ? nops[idx] : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane == 0) wsum[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) { int64_t t = 0; for (int w = 0; w < 16; w++) t += wsum[w]; sums[blockIdx.x] = t; }
}
// block_off[b] = exclusive offset of block b (carry included), from scan_kernel over the sums
__global__ __launch_bounds__(1024) void scan_apply_kernel(const int64_t *__restrict__ nops, int n, const int64_t *__restrict__ block_off, int64_t *__restrict__ off) {
    __shared__ int64_t wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x * 1024 + threadIdx.x;
    const int64_t v = idx < n ? nops[idx] : 0;
    int64_t sum = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int64_t t = __shfl_up(sum, d, 64); if (lane >= d) sum += t; }
    if (lane == 63) wsum[wave] = sum;
    __syncthreads();
    if (wave == 0) {
        int64_t t = lane < 16 ? wsum[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) { const int64_t u = __shfl_up(t, d, 64); if (lane >= d) t += u; }
        if (lane < 16) wsum[lane] = t;
    }
    __syncthreads();
    if (idx < n) off[idx] = block_off[blockIdx.x] + (wave > 0 ? wsum[wave - 1] : 0) + sum - v;
    if (idx == n - 1) off[n] = block_off[blockIdx.x] + (wave > 0 ? wsum[wave - 1] : 0) + sum;
}

// single-pass cooperative traceback (traceback_kernel<.., SCR>): runs staged in traceback order -> dense output, alignment order
__global__ __launch_bounds__(256) void reverse_runs_kernel(const PairPlan *__restrict__ plans, int n_pairs, const gnx_cigar *__restrict__ scr,
                                                            const int64_t *__restrict__ scr_off, const int64_t *__restrict__ nops,
                                                            const int64_t *__restrict__ ops_off, gnx_cigar *__restrict__ ops, int64_t ops_capacity,
                                                            int *__restrict__ err) {
    const int p = blockIdx.x;
    if (p >= n_pairs) return;
    const int po = plans[p].src;
    const int64_t cnt = nops[po], base = ops_off[po], sb = scr_off[p];
    if (base + cnt > ops_capacity) { if (threadIdx.x == 0) atomicOr(err, 4); return; }
    for (int64_t x = threadIdx.x; x < cnt; x += blockDim.x) ops[base + (cnt - 1 - x)] = scr[sb + x];
}

// windows of the packed reference back to bytes: for the kernels of the general and the snapshot paths (run_device), for
// AffineGapLocal on the resident reference (its fast path reads the long sequence as the kernels' alpha) and, with GNX_REF_UNPACK=1,
// for every call (the A/B of the packed reads)
__global__ __launch_bounds__(256) void unpack_windows_kernel(KParams kp, const int64_t *__restrict__ start, const int64_t *__restrict__ out_off, int n_pairs,
                                                             uint8_t *__restrict__ out) {
    const int p = blockIdx.x; // one workgroup per window
    if (p >= n_pairs) return;
    const int64_t len = out_off[p + 1] - out_off[p];
    BetaSrc b;
    b.init(nullptr, kp, start[p], len);
    for (int64_t k = threadIdx.x; k < len; k += blockDim.x) out[out_off[p] + k] = (uint8_t)b.at(k);
}

// CIGAR offsets of a sub-batch (they start at 0) moved behind the runs of the sub-batches before it
__global__ __launch_bounds__(256) void add_offset_kernel(int64_t *__restrict__ off, int64_t n, int64_t base) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) off[x] += base;
}
// gnx_locate_* on the routes that produce a CIGAR: end[p] = target length minus the trailing GNX_COL_D run of pair p's CIGAR
__global__ __launch_bounds__(256) void cigar_target_end_kernel(const gnx_cigar *__restrict__ ops, const int64_t *__restrict__ off, const int64_t *__restrict__ target_len,
                                                               int64_t n, int64_t *__restrict__ end) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int64_t e = target_len[p];
    if (off[p + 1] > off[p]) { const gnx_cigar last = ops[off[p + 1] - 1]; if (last.op == GNX_COL_D) e -= last.run_length; }
    end[p] = e;
}
// gnx_locate_span_* on the same routes: also start[p] = the leading GNX_COL_D run of pair p's CIGAR (0 if it does not begin with one);
// a CIGAR that is ONE GNX_COL_D run (an empty query) gives start = end = 0
__global__ __launch_bounds__(256) void cigar_target_span_kernel(const gnx_cigar *__restrict__ ops, const int64_t *__restrict__ off, const int64_t *__restrict__ target_len,
                                                                int64_t n, int64_t *__restrict__ start, int64_t *__restrict__ end) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    int64_t s = 0, e = target_len[p];
    if (off[p + 1] > off[p]) {
        const gnx_cigar first = ops[off[p]], last = ops[off[p + 1] - 1];
        if (last.op == GNX_COL_D) e -= last.run_length;
        if (first.op == GNX_COL_D && off[p + 1] - off[p] > 1) s = first.run_length;
    }
    start[p] = s;
    end[p] = e;
}

// ---- gnx_best_of_*: reverse complements, per read the first maximum of its candidates, the winners' window tables ---------------
// rc[read_off[r] + k] = complement of reads[read_off[r + 1] - 1 - k]: A <-> T, C <-> G, N stays N, a byte >= 5 stays what it is (and
// still makes GNX_EBASE) -- dna.ReverseComplement on upper-case bases.  One wave per read, four reads per workgroup.
__global__ __launch_bounds__(256) void revcomp_reads_kernel(const uint8_t *__restrict__ reads, const int64_t *__restrict__ read_off, int64_t n_reads,
                                                            uint8_t *__restrict__ rc) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_reads; r += (int64_t)gridDim.x * 4) {
        const int64_t b = read_off[r], e = read_off[r + 1];
        for (int64_t k = b + lane; k < e; k += 64) {
            const uint8_t v = reads[e - 1 - (k - b)];
            rc[k] = v < 4 ? (uint8_t)(3 - v) : v;
        }
    }
}
// best[r] = index, among the candidates cand_off[r] .. cand_off[r + 1] of read r, of the first maximum of score (ties: the lowest
// index); best_score / best_end = that candidate's values (end may be nullptr).  No candidates: -1, 0, 0.  One thread per read.
__global__ __launch_bounds__(256) void first_max_kernel(const int64_t *__restrict__ score, const int64_t *__restrict__ end, const int64_t *__restrict__ cand_off,
                                                        int64_t n_reads, int32_t *__restrict__ best, int64_t *__restrict__ best_score, int64_t *__restrict__ best_end) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const int64_t c0 = cand_off[r], c1 = cand_off[r + 1];
    int64_t at = -1, s = 0;
    for (int64_t c = c0; c < c1; c++) {
        const int64_t v = score[c];
        if (at < 0 || v > s) { at = c; s = v; }
    }
    best[r] = at < 0 ? -1 : (int32_t)(at - c0);
    best_score[r] = s;
    if (end) best_end[r] = at < 0 ? 0 : end[at];
}
// The pair tables of the CIGAR stage: winner w is read win_read[w] with its candidate best[read]; the read's start is the one the
// score stage used (cand_rstart: in the forward or in the reverse-complement copy), the window's start is the candidate's.
__global__ __launch_bounds__(256) void winner_tables_kernel(const int32_t *__restrict__ best, const int64_t *__restrict__ cand_off, const int64_t *__restrict__ win_read,
                                                            const int64_t *__restrict__ cand_rstart, const int64_t *__restrict__ cand_wstart, int64_t n_win,
                                                            int64_t *__restrict__ win_rstart, int64_t *__restrict__ win_wstart) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_win) return;
    const int64_t r = win_read[w], c = cand_off[r] + best[r];
    win_rstart[w] = cand_rstart[c];
    win_wstart[w] = cand_wstart[c];
}

// ---- gnx_best_pair_*: the two mates of a read pair placed together (gnx_align.h states the rule) ----------------------------------
// The wave-wide maximum of (score, then the LOWEST index): at < 0 means "none".  at is unique per item, so the order is total and every
// lane ends with the same winner whatever the lanes held.  64-bit values cross lanes as two 32-bit halves.
struct PairPick { int64_t score, at; };
__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int d) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)v >> 32), d, 64);
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void pick_better(PairPick &k, int64_t score, int64_t at) {
    if (at >= 0 && (k.at < 0 || score > k.score || (score == k.score && at < k.at))) { k.score = score; k.at = at; }
}
__device__ __forceinline__ PairPick wave_pick(PairPick k) {
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t os = shfl_xor_i64(k.score, d), oa = shfl_xor_i64(k.at, d);
        pick_better(k, os, oa);
    }
    return k;
}
// the maximum over the candidates [c0, c1) other than `skip` (an absolute index, or -1), indices relative to c0
__device__ __forceinline__ PairPick wave_first_max(const int64_t *__restrict__ score, int64_t c0, int64_t c1, int64_t skip, int lane) {
    PairPick k{0, -1};
    for (int64_t c = c0 + lane; c < c1; c += 64) if (c != skip) pick_better(k, score[c], c - c0);
    return wave_pick(k);
}
struct PairSelectArgs {
    const int64_t *score, *start, *end, *wstart, *cand_off; // per candidate: the span entry's three values and the window's start
    const uint8_t *strand;
    int64_t n_pairs, min_insert, max_insert, penalty;
    int32_t *best;                                           // per read
    int64_t *best_score, *best_start, *best_end, *second;
    uint8_t *proper;                                         // per pair
    int64_t *tlen;
};
// candidates x of mate 1 and y of mate 2 (absolute indices): E(v) - A(f) if the combination is proper, else -1
__device__ __forceinline__ int64_t proper_insert(const PairSelectArgs &a, int64_t x, int64_t y) {
    if (a.strand[x] == a.strand[y] || a.end[x] <= a.start[x] || a.end[y] <= a.start[y]) return -1;
    const int64_t f = a.strand[x] ? y : x, v = a.strand[x] ? x : y; // f on strand 0, v on strand 1
    const int64_t Af = a.wstart[f] + a.start[f], Ef = a.wstart[f] + a.end[f], Av = a.wstart[v] + a.start[v], Ev = a.wstart[v] + a.end[v];
    if (Af > Av || Ef > Ev || Ev - Af < a.min_insert || Ev - Af > a.max_insert) return -1;
    return Ev - Af;
}
// One wave per read pair (reads 2k, 2k + 1) and per workgroup, so that what is the same for the whole wave (the pair, its offsets, K1, K2)
// is uniform by construction.  The K1 * K2 combinations c = c1 * K2 + c2 are strided over the lanes; each lane keeps its best proper one,
// wave_pick reduces them (ties: the lowest c, i.e. the lowest c1, then the lowest c2).  The same wave finds both mates' first maxima,
// decides, and looks up the runner-up of what it chose.  Lane 0 writes.
__global__ __launch_bounds__(64) void pair_select_kernel(PairSelectArgs a) {
    const int lane = threadIdx.x;
    for (int64_t k = blockIdx.x; k < a.n_pairs; k += gridDim.x) {
        const int64_t b1 = a.cand_off[2 * k], b2 = a.cand_off[2 * k + 1], e2 = a.cand_off[2 * k + 2];
        const int K1 = (int)(b2 - b1), K2 = (int)(e2 - b2); // (out_best is 32 bits wide: K1, K2 < 2^31)
        const PairPick f1 = wave_first_max(a.score, b1, b2, -1, lane), f2 = wave_first_max(a.score, b2, e2, -1, lane);
        // the lane's combinations c = lane, lane + 64, ... as (c1, c2) = (c / K2, c % K2), advanced without a 64-bit division; the key of
        // the reduction is c1 << 32 | c2, which orders the combinations exactly as c does
        int c1 = 0, c2 = lane, step1 = 0, step2 = 64;
        if (K2 > 0 && K2 <= 64) { c1 = lane / K2; c2 = lane % K2; step1 = 64 / K2; step2 = 64 % K2; }
        PairPick p{0, -1};
        while (K2 > 0 && c1 < K1) {
            if (proper_insert(a, b1 + c1, b2 + c2) >= 0) pick_better(p, a.score[b1 + c1] + a.score[b2 + c2], ((int64_t)c1 << 32) | c2);
            c1 += step1;
            unsigned next = (unsigned)c2 + (unsigned)step2; // (below 2^32: c2 < K2 < 2^31 and step2 <= 64)
            if (next >= (unsigned)K2) { next -= (unsigned)K2; c1++; }
            c2 = (int)next;
        }
        const PairPick w = wave_pick(p);
        const bool proper = w.at >= 0 && w.score >= f1.score + f2.score - a.penalty;
        const int at1 = proper ? (int)(w.at >> 32) : (int)f1.at, at2 = proper ? (int)(w.at & 0x7fffffff) : (int)f2.at;
        const PairPick s1 = wave_first_max(a.score, b1, b2, at1 < 0 ? -1 : b1 + at1, lane), s2 = wave_first_max(a.score, b2, e2, at2 < 0 ? -1 : b2 + at2, lane);
        if (lane == 0) {
            const int at[2] = {at1, at2};
            const int64_t base[2] = {b1, b2};
            const PairPick sec[2] = {s1, s2};
            for (int m = 0; m < 2; m++) {
                const int64_t r = 2 * k + m, c = base[m] + at[m];
                a.best[r] = at[m];
                a.best_score[r] = at[m] < 0 ? 0 : a.score[c];
                a.best_start[r] = at[m] < 0 ? 0 : a.start[c];
                a.best_end[r] = at[m] < 0 ? 0 : a.end[c];
                a.second[r] = sec[m].at < 0 ? INT64_MIN : sec[m].score;
            }
            a.proper[k] = proper ? 1 : 0;
            a.tlen[k] = proper ? proper_insert(a, b1 + at1, b2 + at2) : 0;
        }
    }
}

} // namespace
