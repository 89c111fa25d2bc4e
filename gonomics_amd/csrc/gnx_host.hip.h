// gnx_host.hip.h -- host-buffer entry points: pipelined sub-batches, resident reference, sharding over several GPUs of one node
// Part of libgonomics_align_hip.so; included by gnx_align.hip (one translation unit).  See DESIGN.md sections 4.7 and 6.
//
// What a cgo shim calls: host buffers in, host buffers out.  Pairs are independent, so a batch is cut twice:
//   * across the contexts (one per GPU, gnx_init_devices) into contiguous blocks of equal DP cells -- one worker thread per
//     context, no data-path exchange; the shared beta buffer / the resident reference is uploaded once to device 0 and broadcast
//     over RCCL (xGMI), results are gathered on device 0 with grouped ncclSend / ncclRecv and leave through one D2H;
//   * inside a context into sub-batches: while sub-batch k is in the kernels, a stager thread copies the reads of k+1 into
//     pinned memory and starts their H2D on a second stream.  Results accumulate on the device and leave once.
// RCCL is loaded with dlopen on first multi-GPU use: a single-GPU process never touches it.
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <chrono>
#include <map>
#include <thread>
#include <unordered_map>
#include "host_cut.h"

namespace {

// ---- pinned result buffers handed to the caller (gnx_free gives them back to the pool) -----------------------------------------
struct PinPool {
    std::mutex mu;
    std::unordered_map<void *, size_t> live;
    std::multimap<size_t, void *> idle;
    size_t idle_bytes = 0;
    void *get(size_t bytes) {
        size_t cap = 4096;
        while (cap < bytes) cap <<= 1;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = idle.lower_bound(cap);
            if (it != idle.end() && it->first <= 2 * cap) {
                void *p = it->second;
                live[p] = it->first; idle_bytes -= it->first; idle.erase(it);
                return p;
            }
        }
        void *p = nullptr;
        if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        live[p] = cap;
        return p;
    }
    bool put(void *p) { // false: not one of ours
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return false;
        const size_t cap = it->second;
        live.erase(it);
        if (idle_bytes + cap > ((size_t)2 << 30)) { (void)hipHostFree(p); return true; }
        idle.emplace(cap, p); idle_bytes += cap;
        return true;
    }
    void drain() {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : idle) (void)hipHostFree(kv.second);
        idle.clear(); idle_bytes = 0;
    }
};
PinPool g_pool;

// ---- RCCL, loaded on demand -----------------------------------------------------------------------------------------------------
struct RcclApi {
    void *h = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr; // optional: used instead of CommDestroy after a failure
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::vector<ncclComm_t> comms; // one per context when active
};
RcclApi g_rccl;
std::mutex g_api_mu;     // the sharded entry points and the life-cycle calls run one at a time
int g_nctx = 1;          // contexts in use (gnx_init_devices)
bool g_shared_dev = false; // several contexts on one device (flow tests on a 1-GPU box): copies instead of RCCL

int rccl_load() {
    if (g_rccl.h) return GNX_OK;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) { set_err("cannot load librccl.so (%s)", dlerror()); return GNX_EDEVICE; }
#define GNX_SYM(field, name) do { g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name)); if (!g_rccl.field) { set_err("librccl.so lacks %s", name); dlclose(h); return GNX_EDEVICE; } } while (0)
    GNX_SYM(CommInitAll, "ncclCommInitAll"); GNX_SYM(CommDestroy, "ncclCommDestroy"); GNX_SYM(Broadcast, "ncclBroadcast");
    GNX_SYM(Send, "ncclSend"); GNX_SYM(Recv, "ncclRecv"); GNX_SYM(GroupStart, "ncclGroupStart"); GNX_SYM(GroupEnd, "ncclGroupEnd");
    GNX_SYM(GetErrorString, "ncclGetErrorString");
#undef GNX_SYM
    g_rccl.CommAbort = reinterpret_cast<decltype(g_rccl.CommAbort)>(dlsym(h, "ncclCommAbort"));
    g_rccl.h = h;
    return GNX_OK;
}
#define RCCLCHK(call)                                                                                                     \
    do {                                                                                                                  \
        ncclResult_t r_ = (call);                                                                                         \
        if (r_ != ncclSuccess) { set_err("RCCL error: %s", g_rccl.GetErrorString(r_)); return GNX_EDEVICE; }              \
    } while (0)
bool g_rccl_broken = false; // a RCCL call failed in this process: every later exchange uses peer copies (transport 3)
int g_transport = 0;        // what carried the last broadcast / gather, see gnx_timing.transport
double g_bcast_ms = 0;      // broadcast time of the current call
bool rccl_active() { return !g_rccl.comms.empty() && !g_rccl_broken; }
// drop the communicators (after a failure: abort, a destroy may wait for the peers of a collective that never completed)
void rccl_drop_comms() {
    for (ncclComm_t cm : g_rccl.comms) {
        if (!cm) continue;
        if (g_rccl_broken && g_rccl.CommAbort) (void)g_rccl.CommAbort(cm);
        else (void)g_rccl.CommDestroy(cm);
    }
    g_rccl.comms.clear();
}
// after a failed RCCL call (the caller has already closed any open group): remember the text, drain whatever was enqueued, abort
// the communicators, and keep RCCL off until gnx_shutdown -- every later exchange of the process uses peer copies (transport 3)
void rccl_give_up() {
    g_rccl_broken = true;
    fprintf(stderr, "[gnx] %s -- falling back to peer copies until gnx_shutdown\n", g_err);
    for (int d = 0; d < g_nctx; d++) { Ctx &c = ctx_at(d); if (c.inited && hipSetDevice(c.device) == hipSuccess) (void)hipDeviceSynchronize(); }
    (void)hipGetLastError();
    rccl_drop_comms();
    if (ctx_at(0).inited) (void)hipSetDevice(ctx_at(0).device);
}

// the synthetic reference is a pure function of the position (splitmix64), 2 bits per base, an N run of
// 1000 bases every 5e7 -- generated where it is used instead of crossing PCIe
__device__ __host__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// out[0 .. n) = bases [pos0, pos0 + n) of the synthetic reference (pos0 a multiple of 32)
__global__ __launch_bounds__(256) void synth_ref_kernel(uint8_t *__restrict__ out, int64_t pos0, int64_t n, uint64_t seed) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // 32 bases per thread: one 64-bit draw
    const int64_t p0 = w * 32;
    if (p0 >= n) return;
    const uint64_t bits = splitmix64(seed ^ (uint64_t)(pos0 / 32 + w));
    for (int k = 0; k < 32 && p0 + k < n; k++) {
        const int64_t pos = pos0 + p0 + k;
        out[p0 + k] = (pos % 50000000 < 1000 && pos >= 50000000) ? 4 : (uint8_t)((bits >> (2 * k)) & 3u);
    }
}

// ---- the resident reference, packed --------------------------------------------------------------------------------------------
// 2 bits per base (A C G T), 16 bases per dword; one flag bit per 64-base block that holds anything else (N = 4, or a byte >= 5 that
// the Go code would panic on WHEN AN ALIGNMENT TOUCHES IT -- so it is recorded, not refused), the rank of every flag word, and per
// flagged block the two masks.  4.4e9 bases: 1.1 GB + 13 MB + 16 B per flagged block, instead of 4.4 GB.
size_t ref_words(int64_t len) { return (size_t)((len + 15) / 16) + 4; }
size_t ref_flagwords(int64_t len) { return (size_t)(((len + 63) / 64 + 63) / 64) + 2; }
constexpr int64_t REF_CHUNK = (int64_t)256 << 20; // bases packed per pass (multiple of 4096): staging 256 MB

// pass 1: one thread per 64-base block of the chunk: the four 2-bit words, the block's flag bit
__global__ __launch_bounds__(256) void pack_ref_kernel(const uint8_t *__restrict__ bytes, int64_t base0, int64_t n, unsigned *__restrict__ w2,
                                                       unsigned long long *__restrict__ flag) {
    const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // block index inside the chunk
    if (blk * 64 >= n) return;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    bool exc = false;
    for (int k = 0; k < 64; k++) {
        const int64_t x = blk * 64 + k;
        const int b = x < n ? bytes[x] : 0;
        if (b >= 4) exc = true;
        w[k >> 4] |= (unsigned)(b & 3) << (2 * (k & 15));
    }
    const int64_t gblk = base0 / 64 + blk;
    unsigned *dst = w2 + gblk * 4;
    dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2]; dst[3] = w[3];
    if (exc) atomicOr(&flag[gblk >> 6], 1ull << (gblk & 63));
}
// pass 2 (ranks known): the masks of the flagged blocks of the chunk
__global__ __launch_bounds__(256) void pack_exc_kernel(const uint8_t *__restrict__ bytes, int64_t base0, int64_t n, const unsigned long long *__restrict__ flag,
                                                       const unsigned *__restrict__ rank, unsigned long long *__restrict__ exc) {
    const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (blk * 64 >= n) return;
    const int64_t gblk = base0 / 64 + blk;
    const unsigned long long f = flag[gblk >> 6];
    if (!((f >> (gblk & 63)) & 1ull)) return;
    unsigned long long nm = 0, bm = 0;
    for (int k = 0; k < 64; k++) {
        const int64_t x = blk * 64 + k;
        const int b = x < n ? bytes[x] : 0;
        if (b == 4) nm |= 1ull << k;
        if (b >= 5) bm |= 1ull << k;
    }
    const int64_t e = (int64_t)rank[gblk >> 6] + __popcll(f & ((1ull << (gblk & 63)) - 1ull));
    exc[2 * e] = nm; exc[2 * e + 1] = bm;
}
int64_t g_ref_epoch = 0;
int ensure_reference(int nc);
// ref != nullptr: host bytes; else the synthetic reference of SURVEY 8d (generated chunk by chunk on the device)
int set_reference_packed(const uint8_t *ref, int64_t len, uint64_t seed) {
    g_ref_epoch++;
    Ctx &c0 = ctx_at(0);
    {
        CtxScope sc(c0);
        int rc = ensure_init();
        if (rc) return rc;
        HIPCHK(hipSetDevice(c0.device));
        hipStream_t st = c0.own_stream;
        c0.ref_len = -1;
        drop_reference_index(c0); // (before anything can fail: an index never outlives the reference it was built from)
        drop_pile(c0);            // (nor does a pile)
        if (len == 0) { // release: every context gives the reference (and the unpacked-window scratch) back; nothing is re-allocated
            int n_all0; { std::lock_guard<std::mutex> lk(g_ctxs_mu); n_all0 = (int)g_ctxs.size(); }
            for (int d = 0; d < n_all0; d++) {
                Ctx &c = ctx_at(d);
                if (!c.inited) continue;
                std::unique_lock<std::mutex> lkd;
                if (d > 0) lkd = std::unique_lock<std::mutex>(c.mu); // (context 0 is held by this call's scope)
                HIPCHK(hipSetDevice(c.device));
                HIPCHK(hipDeviceSynchronize());
                c.ref.release(); c.ref_flag.release(); c.ref_rank.release(); c.ref_exc.release(); c.unpk_b.release(); c.unpk_off.release();
                c.ref_len = -1;
            }
            HIPCHK(hipSetDevice(c0.device));
            g_bcast_ms = 0;
            return GNX_OK;
        }
        const size_t nw = ref_words(len), nf = ref_flagwords(len);
        if ((rc = c0.ref.ensure(nw * 4))) return rc;
        if ((rc = c0.ref_flag.ensure(nf * 8))) return rc;
        if ((rc = c0.ref_rank.ensure(nf * 4))) return rc;
        HIPCHK(hipMemsetAsync(c0.ref.p, 0, nw * 4, st));
        HIPCHK(hipMemsetAsync(c0.ref_flag.p, 0, nf * 8, st));
        DevBuf stage;
        const int64_t chunk = std::min<int64_t>(REF_CHUNK, std::max<int64_t>(len, 1));
        if ((rc = stage.ensure((size_t)chunk + 64))) return rc;
        std::vector<unsigned long long> hflag(nf, 0ull);
        std::vector<unsigned> hrank(nf, 0u);
        int64_t nexc = 0;
        // exception masks: grown as needed (a genome's N runs are a few per cent of its blocks at most)
        auto grow_exc = [&](int64_t want, int64_t keep) -> int {
            if ((size_t)want * 16 <= c0.ref_exc.cap) return GNX_OK;
            DevBuf nb;
            int r = nb.ensure((size_t)std::max<int64_t>(want * 2, 1024) * 16);
            if (r) return r;
            if (keep > 0) { HIPCHK(hipMemcpyAsync(nb.p, c0.ref_exc.p, (size_t)keep * 16, hipMemcpyDeviceToDevice, st)); HIPCHK(hipStreamSynchronize(st)); }
            c0.ref_exc.release(); c0.ref_exc = nb;
            return GNX_OK;
        };
        if ((rc = grow_exc(1, 0))) { stage.release(); return rc; }
        auto fail = [&](int code) { stage.release(); return code; };
        for (int64_t b0 = 0; b0 < len; b0 += chunk) {
            const int64_t n = std::min(chunk, len - b0);
            if (ref) { if (hipMemcpyAsync(stage.p, ref + b0, (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess) { set_err("upload of the reference failed%s", ""); return fail(GNX_EDEVICE); } }
            else hipLaunchKernelGGL(synth_ref_kernel, dim3((unsigned)(((n + 31) / 32 + 255) / 256)), dim3(256), 0, st, (uint8_t *)stage.p, b0, n, seed);
            const int64_t nblk = (n + 63) / 64;
            hipLaunchKernelGGL(pack_ref_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, (const uint8_t *)stage.p, b0, n, (unsigned *)c0.ref.p, (unsigned long long *)c0.ref_flag.p);
            // ranks of this chunk's flag words (the chunk starts on a flag-word boundary: REF_CHUNK is a multiple of 4096)
            const size_t f0 = (size_t)(b0 / 4096), f1 = (size_t)((b0 + n + 4095) / 4096);
            if (hipMemcpyAsync(hflag.data() + f0, (const unsigned long long *)c0.ref_flag.p + f0, (f1 - f0) * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { set_err("packing the reference failed%s", ""); return fail(GNX_EDEVICE); }
            const int64_t before = nexc;
            for (size_t f = f0; f < f1; f++) { hrank[f] = (unsigned)nexc; nexc += __builtin_popcountll(hflag[f]); }
            if (nexc > 0xfffffff0LL) { set_err("too many non-ACGT blocks in the reference%s", ""); return fail(GNX_ENOMEM); }
            if (nexc > before) {
                if ((rc = grow_exc(nexc, before))) return fail(rc);
                if (hipMemcpyAsync((unsigned *)c0.ref_rank.p + f0, hrank.data() + f0, (f1 - f0) * 4, hipMemcpyHostToDevice, st) != hipSuccess) { set_err("packing the reference failed%s", ""); return fail(GNX_EDEVICE); }
                hipLaunchKernelGGL(pack_exc_kernel, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, st, (const uint8_t *)stage.p, b0, n, (const unsigned long long *)c0.ref_flag.p,
                                   (const unsigned *)c0.ref_rank.p, (unsigned long long *)c0.ref_exc.p);
            }
            if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) { set_err("packing the reference failed%s", ""); return fail(GNX_EDEVICE); }
        }
        // the ranks of ALL flag words (also behind the last chunk: BetaSrc::init looks one block past a window's end)
        for (size_t f = (size_t)((len + 4095) / 4096); f < nf; f++) hrank[f] = (unsigned)nexc;
        if (hipMemcpy(c0.ref_rank.p, hrank.data(), nf * 4, hipMemcpyHostToDevice) != hipSuccess) { set_err("packing the reference failed%s", ""); return fail(GNX_EDEVICE); }
        stage.release();
        c0.ref_len = len; c0.ref_nexc = nexc; c0.ref_epoch = g_ref_epoch;
    }
    // contexts beyond the ones in use no longer hold the current reference; the others get it now
    int n_all; { std::lock_guard<std::mutex> lk(g_ctxs_mu); n_all = (int)g_ctxs.size(); }
    for (int d = 1; d < n_all; d++) { Ctx &c = ctx_at(d); CtxScope sc(c); c.ref_len = -1; }
    g_bcast_ms = 0;
    return ensure_reference(g_nctx);
}

// ---- one context's share of a batch ---------------------------------------------------------------------------------------------
struct SeqSide { // one sequence per pair: a window (start, len) of buf, or of the resident reference
    const uint8_t *buf;
    int64_t buf_len;
    const int64_t *start, *len;
    bool resident;
};
struct HostWant { // what a host call gives back beside the scores, and which side plays which role
    bool cigars = true;          // false: gnx_score_* / gnx_locate_* (the score sweep, or the ordinary route with its CIGAR left on the device)
    int64_t *end = nullptr;      // gnx_locate_* (AffineGapLocal, no CIGARs): the target end of every pair
    int64_t *start = nullptr;    // gnx_locate_span_* (with end): the target start as well
    bool query_is_alpha = false; // with end: alpha = query, beta = target (windows of the resident reference); else alpha = target, beta = query
};
struct HostJob {
    Ctx *c = nullptr;
    const gnx_params *prm = nullptr;
    int64_t p0 = 0, p1 = 0; // pairs [p0, p1) of the call
    SeqSide a = {}, b = {};  // host windows; b.resident: windows into b_dev
    HostWant want;           // (end / start: asked for or not -- the values stay on the device until the gather)
    const uint8_t *b_dev = nullptr; // != nullptr: the whole beta buffer / the resident reference is on this context's device
    bool packed = false;            // b_dev is the PACKED resident reference (beta windows = base positions in it)
    int64_t total_ops = 0;
    int rc = GNX_OK;
    char err[512] = "";
    gnx_timing timing = {};
};

int grow_ops(Ctx &c, int64_t keep_elems, int64_t want_elems, hipStream_t st) {
    if ((size_t)want_elems * sizeof(gnx_cigar) <= c.res_ops.cap) return GNX_OK;
    DevBuf nb;
    int rc = nb.ensure((size_t)want_elems * sizeof(gnx_cigar));
    if (rc) return rc;
    if (keep_elems > 0) {
        HIPCHK(hipMemcpyAsync(nb.p, c.res_ops.p, (size_t)keep_elems * sizeof(gnx_cigar), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    c.res_ops.release();
    c.res_ops = nb;
    return GNX_OK;
}

// While one lives, run_device and run_score_sweep read the context's beta windows as positions in its packed reference
// (Ctx::beta_packed, when `on`); the flag is down again on every way out of the scope.
struct PackedBeta {
    Ctx &c;
    PackedBeta(Ctx &c_, bool on) : c(c_) { c.beta_packed = on; }
    ~PackedBeta() { c.beta_packed = false; }
};

// sum += the device timing of one sub-batch; fast_path: the last sub-batch's, or the largest code seen (the score-only flows)
void add_timing(gnx_timing &sum, const gnx_timing &t, bool max_fast_path) {
    sum.fill_ms += t.fill_ms; sum.traceback_ms += t.traceback_ms; sum.total_ms += t.total_ms; sum.cells += t.cells;
    sum.n_launches += t.n_launches; sum.trace_bytes += t.trace_bytes; sum.dominant_ms += t.dominant_ms;
    sum.dominant_launches += t.dominant_launches; sum.fast_path = max_fast_path ? std::max(sum.fast_path, t.fast_path) : t.fast_path;
}

// `cnt` windows of the context's packed reference (device starts, host lengths) as bytes in c.in_b, their offsets in c.in_bl
// (AffineGapLocal off the sweep reads its target as the kernels' alpha; GNX_REF_UNPACK: A/B)
int unpack_ref_windows(Ctx &c, const int64_t *d_starts, const int64_t *h_lens, int64_t cnt, hipStream_t st) {
    std::vector<int64_t> uoff((size_t)cnt + 1, 0);
    for (int64_t q = 0; q < cnt; q++) uoff[(size_t)q + 1] = uoff[(size_t)q] + h_lens[q];
    int r;
    if ((r = c.in_b.ensure((size_t)uoff[(size_t)cnt] + 64)) || (r = c.in_bl.ensure((size_t)(cnt + 1) * 8))) return r;
    KParams ukp;
    memset(&ukp, 0, sizeof(ukp));
    ukp.b2 = (const unsigned *)c.ref.p; ukp.bflag = (const unsigned long long *)c.ref_flag.p; ukp.brank = (const unsigned *)c.ref_rank.p; ukp.bexc = (const unsigned long long *)c.ref_exc.p;
    HIPCHK(hipMemcpyAsync(c.in_bl.p, uoff.data(), (size_t)(cnt + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (uoff is a local)
    hipLaunchKernelGGL(unpack_windows_kernel, dim3((unsigned)cnt), dim3(256), 0, st, ukp, d_starts, (const int64_t *)c.in_bl.p, (int)cnt, (uint8_t *)c.in_b.p);
    HIPCHK(hipGetLastError());
    return GNX_OK;
}

// A batch of a score-only call on the current context: the score sweep where it applies (run_score_sweep), else the ordinary
// route, whose CIGAR goes into the context's result buffer and simply stays there.  Sets c.timing like run_device.
// d_end != nullptr (gnx_locate_*, alpha = target): also the target end of every pair, from the sweep or read off the CIGAR on the
// device.  d_start != nullptr (gnx_locate_span_*, with d_end): the target start as well, from stage 2 behind the sweep (fast_path 10) or off the
// CIGAR.  try_sweep = false: the caller has tried the sweep already.
int score_or_fallback(Ctx &c, const gnx_params *prm, int64_t cnt, const uint8_t *d_a, const int64_t *d_as, const uint8_t *d_b, const int64_t *d_bs,
                      const int64_t *h_alen, const int64_t *h_blen, int64_t *d_score, hipStream_t stream, int64_t *d_end = nullptr, bool try_sweep = true,
                      int64_t *d_start = nullptr) {
    int rc = try_sweep ? run_score_sweep(prm, cnt, d_a, d_as, d_b, d_bs, h_alen, h_blen, d_score, stream, d_end, false, d_start) : -1;
    if (rc != -1) return rc;
    if ((rc = c.ss_off.ensure((size_t)(std::max<int64_t>(cnt, 0) + 1) * 8))) return rc;
    if ((rc = grow_ops(c, 0, std::max<int64_t>((int64_t)1 << 20, 64 * cnt), stream))) return rc;
    int64_t tot = 0;
    for (int attempt = 0;; attempt++) {
        rc = run_device(prm, cnt, d_a, d_as, d_b, d_bs, h_alen, h_blen, d_score, (gnx_cigar *)c.res_ops.p, (int64_t)(c.res_ops.cap / sizeof(gnx_cigar)), (int64_t *)c.ss_off.p, &tot, stream);
        if (rc != GNX_ECAPACITY || attempt >= 8) break;
        if ((rc = grow_ops(c, 0, tot + 1024, stream))) break;
    }
    if (rc == GNX_OK && d_end && cnt > 0) {
        if ((rc = c.ss_len.ensure((size_t)cnt * 8))) return rc;
        HIPCHK(hipMemcpyAsync(c.ss_len.p, h_alen, (size_t)cnt * 8, hipMemcpyHostToDevice, stream));
        if (d_start) hipLaunchKernelGGL(cigar_target_span_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, (const gnx_cigar *)c.res_ops.p, (const int64_t *)c.ss_off.p,
                                        (const int64_t *)c.ss_len.p, cnt, d_start, d_end);
        else hipLaunchKernelGGL(cigar_target_end_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, (const gnx_cigar *)c.res_ops.p, (const int64_t *)c.ss_off.p,
                                (const int64_t *)c.ss_len.p, cnt, d_end);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream)); // h_alen is the caller's
    }
    return rc;
}

// AffineGapLocal without CIGARs, the reads (queries) as the kernels' alpha against target windows as their beta: the sweep as it
// is (query_is_alpha), reading the windows where they are -- `packed`: in the packed reference; off the sweep the ordinary route
// with the two sides swapped, which wants the windows as bytes.
int locate_reads_in_windows(Ctx &c, const gnx_params *prm, int64_t cnt, const uint8_t *d_reads, const int64_t *d_rs, const int64_t *h_rlen,
                            const uint8_t *d_win, const int64_t *d_ws, const int64_t *h_wlen, bool packed, int64_t *d_score, int64_t *d_end, int64_t *d_start, hipStream_t st) {
    int rc;
    { PackedBeta pb(c, packed); rc = run_score_sweep(prm, cnt, d_reads, d_rs, d_win, d_ws, h_rlen, h_wlen, d_score, st, d_end, true, d_start); }
    if (rc != -1) return rc;
    if (packed) {
        if ((rc = unpack_ref_windows(c, d_ws, h_wlen, cnt, st))) return rc;
        d_win = (const uint8_t *)c.in_b.p; d_ws = (const int64_t *)c.in_bl.p;
    }
    return score_or_fallback(c, prm, cnt, d_win, d_ws, d_reads, d_rs, h_wlen, h_rlen, d_score, st, d_end, false, d_start);
}

// The CIGAR tail of one sub-batch, pairs [done, done + cnt) of n: `run(d_score, d_ops, cap, d_off, &tot)` is the flow's run_device
// call (the flows differ in which side is alpha), writing scores and offsets at `done` of the context's result buffers and runs
// behind the `total` kept so far.  GNX_ECAPACITY grows the run buffer and tries again; then the offsets, which a sub-batch counts
// from 0, are rebased and `total` moves on.
template <class Run>
int run_sub_batch_cigars(Ctx &c, int64_t n, int64_t done, int64_t cnt, int64_t &total, hipStream_t st, Run run) {
    int64_t tot = 0;
    int rc;
    for (int attempt = 0;; attempt++) {
        const int64_t cap = (int64_t)(c.res_ops.cap / sizeof(gnx_cigar)) - total;
        rc = run((int64_t *)c.res_score.p + done, (gnx_cigar *)c.res_ops.p + total, cap, (int64_t *)c.res_off.p + done, &tot);
        if (rc != GNX_ECAPACITY || attempt >= 8) break;
        // the reported total is exact (every sub-batch of the device flow is counted); leave room for the sub-batches to come
        const int64_t left = (n - done + cnt - 1) / cnt;
        if ((rc = grow_ops(c, total, total + tot * std::min<int64_t>(left, 4) + 1024, st))) break;
    }
    if (rc) return rc;
    if (total > 0) {
        hipLaunchKernelGGL(add_offset_kernel, dim3((unsigned)((cnt + 1 + 255) / 256)), dim3(256), 0, st, (int64_t *)c.res_off.p + done, cnt + 1, total);
        HIPCHK(hipGetLastError());
    }
    total += tot;
    return GNX_OK;
}

// runs on the thread that owns the context (t_ctx == job.c, device current)
int run_host_job(HostJob &j) {
    Ctx &c = *j.c;
    const int64_t n = j.p1 - j.p0;
    int rc;
    if ((rc = c.res_score.ensure((size_t)std::max<int64_t>(n, 1) * 8))) return rc;
    if ((rc = c.res_off.ensure((size_t)(n + 1) * 8))) return rc;
    if (j.want.end && (rc = c.res_end.ensure((size_t)std::max<int64_t>(n, 1) * 8))) return rc;
    if (j.want.start && (rc = c.res_start.ensure((size_t)std::max<int64_t>(n, 1) * 8))) return rc;
    if (n == 0) { HIPCHK(hipMemsetAsync(c.res_off.p, 0, 8, c.own_stream)); HIPCHK(hipStreamSynchronize(c.own_stream)); return GNX_OK; }
    const int64_t size = sub_batch_size(n, gnx_host_sub(getenv("GNX_HOST_SUB")));
    const int64_t K = (n + size - 1) / size;
    const int64_t *as = j.a.start + j.p0, *al = j.a.len + j.p0, *bs = j.b.start + j.p0, *bl = j.b.len + j.p0;

    // stage(k): inputs of sub-batch k -> device buffers of slot k & 1 (H2D on s_in, event ev_in[slot]).  k == 0 copies straight from
    // the caller's memory (nothing to overlap with); later ones go through pinned memory so that the DMA runs under the kernels.
    std::vector<int64_t> tmp_as, tmp_bs;
    int stage_rc = GNX_OK;
    char stage_err[512] = "";
    auto stage = [&](int64_t k, bool pinned) -> int {
        const int slot = (int)(k & 1);
        const int64_t b = k * size, e = std::min(n, b + size), cnt = e - b;
        int64_t alo = INT64_MAX, ahi = 0, blo = INT64_MAX, bhi = 0;
        for (int64_t q = b; q < e; q++) {
            alo = std::min(alo, as[q]); ahi = std::max(ahi, as[q] + al[q]);
            if (!j.b_dev) { blo = std::min(blo, bs[q]); bhi = std::max(bhi, bs[q] + bl[q]); }
        }
        if (ahi < alo) { alo = 0; ahi = 0; }
        if (bhi < blo) { blo = 0; bhi = 0; }
        int r;
        if ((r = c.pin_a[slot].ensure((size_t)(ahi - alo) + 16))) return r;
        if ((r = c.pin_as[slot].ensure((size_t)cnt * 8))) return r;
        if ((r = c.pin_bs[slot].ensure((size_t)cnt * 8))) return r;
        if (!j.b_dev && (r = c.pin_b[slot].ensure((size_t)(bhi - blo) + 16))) return r;
        int64_t *has, *hbs;
        const uint8_t *src_a = j.a.buf + alo, *src_b = j.b_dev ? nullptr : j.b.buf + blo;
        if (pinned) {
            if ((r = c.st_a[slot].ensure((size_t)(ahi - alo) + 16))) return r;
            if ((r = c.st_as[slot].ensure((size_t)cnt * 8))) return r;
            if ((r = c.st_bs[slot].ensure((size_t)cnt * 8))) return r;
            if (!j.b_dev && (r = c.st_b[slot].ensure((size_t)(bhi - blo) + 16))) return r;
            memcpy(c.st_a[slot].p, src_a, (size_t)(ahi - alo)); src_a = (const uint8_t *)c.st_a[slot].p;
            if (!j.b_dev) { memcpy(c.st_b[slot].p, src_b, (size_t)(bhi - blo)); src_b = (const uint8_t *)c.st_b[slot].p; }
            has = (int64_t *)c.st_as[slot].p; hbs = (int64_t *)c.st_bs[slot].p;
        } else {
            tmp_as.resize((size_t)cnt); tmp_bs.resize((size_t)cnt);
            has = tmp_as.data(); hbs = tmp_bs.data();
        }
        for (int64_t q = 0; q < cnt; q++) { has[q] = as[b + q] - alo; hbs[q] = j.b_dev ? bs[b + q] : bs[b + q] - blo; }
        if (ahi > alo) HIPCHK(hipMemcpyAsync(c.pin_a[slot].p, src_a, (size_t)(ahi - alo), hipMemcpyHostToDevice, c.s_in));
        if (!j.b_dev && bhi > blo) HIPCHK(hipMemcpyAsync(c.pin_b[slot].p, src_b, (size_t)(bhi - blo), hipMemcpyHostToDevice, c.s_in));
        HIPCHK(hipMemcpyAsync(c.pin_as[slot].p, has, (size_t)cnt * 8, hipMemcpyHostToDevice, c.s_in));
        HIPCHK(hipMemcpyAsync(c.pin_bs[slot].p, hbs, (size_t)cnt * 8, hipMemcpyHostToDevice, c.s_in));
        if (!pinned) HIPCHK(hipStreamSynchronize(c.s_in)); // tmp_* / the caller's pageable memory: do not rely on the staging
        HIPCHK(hipEventRecord(c.ev_in[slot], c.s_in));
        return GNX_OK;
    };

    const auto t_stage = std::chrono::steady_clock::now();
    if ((rc = stage(0, false))) return rc;
    const double stage0_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_stage).count();
    int64_t done = 0, total = 0;
    // CIGAR capacity: a guess that fits every workload of the path's callers, grown (with a retry of the sub-batch) when it does not
    int64_t worst = 0;
    for (int64_t q = 0; q < n; q++) worst += al[q] + bl[q] + 1;
    if (j.want.cigars && (rc = grow_ops(c, 0, std::max<int64_t>(std::min<int64_t>(worst, std::max<int64_t>((int64_t)1 << 20, 64 * std::min(n, size))), 1), c.own_stream))) return rc;
    gnx_timing tsum = {};
    for (int64_t k = 0; k < K; k++) {
        const int slot = (int)(k & 1);
        const int64_t b = k * size, e = std::min(n, b + size), cnt = e - b;
        std::thread stager;
        if (k + 1 < K) {
            stager = std::thread([&, k]() {
                t_ctx = &c;
                if (hipSetDevice(c.device) != hipSuccess) { stage_rc = GNX_EDEVICE; return; }
                g_err[0] = 0;
                stage_rc = stage(k + 1, true);
                if (stage_rc) memcpy(stage_err, g_err, sizeof(stage_err));
            });
        }
        // the sub-batch on the device (no return past the stager: it is joined below)
        auto run_sub = [&]() -> int {
            if (hipStreamWaitEvent(c.own_stream, c.ev_in[slot], 0) != hipSuccess) { set_err("hipStreamWaitEvent failed%s", ""); return GNX_EDEVICE; }
            const uint8_t *da = (const uint8_t *)c.pin_a[slot].p, *db = j.b_dev ? j.b_dev : (const uint8_t *)c.pin_b[slot].p;
            const int64_t *das = (const int64_t *)c.pin_as[slot].p, *dbs = (const int64_t *)c.pin_bs[slot].p;
            int64_t *d_sc = (int64_t *)c.res_score.p + done, *d_en = j.want.end ? (int64_t *)c.res_end.p + done : nullptr, *d_st = j.want.start ? (int64_t *)c.res_start.p + done : nullptr;
            bool packed = j.packed;
            int r;
            if (j.want.end && j.want.query_is_alpha) // (gnx_locate_batch_by_offset: the local sweep reads its target packed; only its fallback needs bytes)
                r = locate_reads_in_windows(c, j.prm, cnt, da, das, al + b, db, dbs, bl + b, packed, d_sc, d_en, d_st, c.own_stream);
            else {
                // the windows as bytes (AffineGapLocal's transposed fast path reads the long sequence as the kernels' alpha; GNX_REF_UNPACK: A/B)
                if (packed && (j.prm->mode == GNX_AFFINE_GAP_LOCAL || getenv("GNX_REF_UNPACK"))) {
                    if ((r = unpack_ref_windows(c, dbs, bl + b, cnt, c.own_stream))) return r;
                    db = (const uint8_t *)c.in_b.p; dbs = (const int64_t *)c.in_bl.p; packed = false;
                }
                PackedBeta pb(c, packed);
                if (!j.want.cigars) r = score_or_fallback(c, j.prm, cnt, da, das, db, dbs, al + b, bl + b, d_sc, c.own_stream, d_en, true, d_st);
                else r = run_sub_batch_cigars(c, n, done, cnt, total, c.own_stream, [&](int64_t *d_score, gnx_cigar *d_ops, int64_t cap, int64_t *d_off, int64_t *tot) {
                    return run_device(j.prm, cnt, da, das, db, dbs, al + b, bl + b, d_score, d_ops, cap, d_off, tot, c.own_stream);
                });
            }
            if (r) return r;
            add_timing(tsum, c.timing, !j.want.cigars);
            done += cnt;
            return GNX_OK;
        };
        rc = run_sub();
        if (stager.joinable()) stager.join();
        if (rc) return rc;
        if (stage_rc) { memcpy(g_err, stage_err, sizeof(stage_err)); publish_err(); return stage_rc; }
    }
    HIPCHK(hipStreamSynchronize(c.own_stream));
    j.total_ops = total;
    tsum.stage0_ms = stage0_ms;
    j.timing = tsum;
    c.timing = tsum;
    return GNX_OK;
}

// contiguous blocks of (nearly) equal DP cells, 8-aligned so that waves stay whole
std::vector<int64_t> partition_by_cells(const int64_t *a_len, const int64_t *b_len, int64_t n, int parts) {
    std::vector<int64_t> bounds((size_t)parts + 1, n);
    bounds[0] = 0;
    if (parts <= 1 || n == 0) return bounds;
    long double total = 0;
    for (int64_t q = 0; q < n; q++) total += (long double)a_len[q] * (long double)b_len[q];
    long double acc = 0;
    int next = 1;
    for (int64_t q = 0; q < n && next < parts; q++) {
        acc += (long double)a_len[q] * (long double)b_len[q];
        while (next < parts && acc >= total * next / parts) { bounds[(size_t)next] = std::min<int64_t>(n, (q + 1 + 7) & ~(int64_t)7); next++; }
    }
    for (int r = 1; r <= parts; r++) bounds[(size_t)r] = std::max(bounds[(size_t)r], bounds[(size_t)r - 1]);
    bounds[(size_t)parts] = n;
    return bounds;
}

// broadcast `bytes` from context 0's buffer src0 to dst[d] of every other context (RCCL over xGMI; plain copies when the contexts
// share a device or RCCL is off)
// GNX_RCCL_INJECT_FAIL=1: the next RCCL exchange reports a failure before it starts; =2: INSIDE its group, after the first operation
// has been enqueued (tests of the fall-back to peer copies; `where` = 1 before ncclGroupStart, 2 inside the group)
bool rccl_injected_failure(int where) {
    const char *e = getenv("GNX_RCCL_INJECT_FAIL");
    if (!e || atoi(e) != where) return false;
    set_err("RCCL error: injected failure (GNX_RCCL_INJECT_FAIL=%s)", e);
    return true;
}
// A grouped exchange: `body` enqueues the operations between ncclGroupStart and ncclGroupEnd.  Whatever fails inside the group, the
// group is CLOSED again before the error is reported (an open group would swallow the next ncclCommInitAll of this thread) and the
// current device is context 0's; the caller then gives RCCL up and repeats the exchange with peer copies.
template <class Body>
int rccl_grouped(Body body) {
    if (rccl_injected_failure(1)) return GNX_EDEVICE;
    RCCLCHK(g_rccl.GroupStart());
    const int rc = body();
    const ncclResult_t re = g_rccl.GroupEnd(); // also on the error path; its own result only matters when the body was fine
    (void)hipSetDevice(ctx_at(0).device);
    if (rc) return rc;
    if (re != ncclSuccess) { set_err("RCCL error: %s", g_rccl.GetErrorString(re)); return GNX_EDEVICE; }
    return GNX_OK;
}
int broadcast_rccl(const void *src0, std::vector<void *> &dst, size_t bytes) {
    const int nc = (int)dst.size();
    int rc = rccl_grouped([&]() -> int {
        for (int d = 0; d < nc; d++) {
            Ctx &c = ctx_at(d);
            HIPCHK(hipSetDevice(c.device));
            RCCLCHK(g_rccl.Broadcast(src0, d == 0 ? const_cast<void *>(src0) : dst[(size_t)d], bytes, ncclUint8, 0, g_rccl.comms[(size_t)d], c.own_stream));
            if (d == 0 && rccl_injected_failure(2)) return GNX_EDEVICE;
        }
        return GNX_OK;
    });
    if (rc) return rc;
    for (int d = 0; d < nc; d++) { Ctx &c = ctx_at(d); HIPCHK(hipSetDevice(c.device)); HIPCHK(hipStreamSynchronize(c.own_stream)); }
    HIPCHK(hipSetDevice(ctx_at(0).device));
    return GNX_OK;
}
int broadcast_from_ctx0(const void *src0, std::vector<void *> &dst, size_t bytes) {
    const int nc = (int)dst.size();
    if (bytes == 0 || nc == 0) return GNX_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // RCCL needs every rank of the communicator in the collective: a call that uses fewer contexts than gnx_init_devices created
    // (a batch too small to cut) copies instead
    bool via_rccl = rccl_active() && (int)g_rccl.comms.size() == nc; // (also with one rank: a no-op that checks the plumbing)
    const bool tried = via_rccl;
    if (via_rccl && broadcast_rccl(src0, dst, bytes) != GNX_OK) { rccl_give_up(); via_rccl = false; }
    if (!via_rccl) for (int d = 1; d < nc; d++) if (dst[(size_t)d] != src0) HIPCHK(hipMemcpyPeer(dst[(size_t)d], ctx_at(d).device, src0, ctx_at(0).device, bytes));
    HIPCHK(hipSetDevice(ctx_at(0).device));
    if (nc > 1 || tried) g_transport = via_rccl ? 1 : (g_rccl_broken ? 3 : 2);
    g_bcast_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GNX_OK;
}
// the resident reference on contexts [0, nc): a context that lacks the current one (created after gnx_set_reference -- ADVICE r2 --
// or simply not context 0, where the packing happens) gets its copy from context 0: four arrays, RCCL over xGMI or peer copies
int ensure_reference(int nc) {
    Ctx &c0 = ctx_at(0);
    if (c0.ref_len < 0) return GNX_OK;
    const size_t sz[4] = {ref_words(c0.ref_len) * 4, ref_flagwords(c0.ref_len) * 8, ref_flagwords(c0.ref_len) * 4, (size_t)std::max<int64_t>(c0.ref_nexc, 1) * 16};
    bool missing = false;
    std::vector<void *> dst[4];
    for (int k = 0; k < 4; k++) dst[k].assign((size_t)nc, nullptr);
    for (int d = 0; d < nc; d++) {
        Ctx &c = ctx_at(d);
        CtxScope sc(c);
        int rc = ensure_init();
        if (rc) return rc;
        DevBuf *bufs[4] = {&c.ref, &c.ref_flag, &c.ref_rank, &c.ref_exc};
        if (d > 0 && (c.ref_len != c0.ref_len || c.ref_epoch != c0.ref_epoch || c.ref.p == nullptr)) {
            missing = true;
            for (int k = 0; k < 4; k++) if ((rc = bufs[k]->ensure(sz[k]))) { c.ref_len = -1; return rc; }
            c.ref_len = c0.ref_len; c.ref_nexc = c0.ref_nexc; c.ref_epoch = c0.ref_epoch;
        }
        for (int k = 0; k < 4; k++) dst[k][(size_t)d] = bufs[k]->p;
    }
    if (!missing) return GNX_OK;
    for (int k = 0; k < 4; k++) { int rc = broadcast_from_ctx0(dst[k][0], dst[k], sz[k]); if (rc) return rc; }
    return GNX_OK;
}

// The sharded host flow.  b.resident: beta windows index the resident reference (gnx_set_reference).
int run_host_sharded(const gnx_params *prm, int64_t n_pairs, const SeqSide &a, const SeqSide &b, int64_t *out_score, gnx_cigar **out_ops, int64_t **out_ops_off,
                     const HostWant &want = HostWant()) {
    const bool score_only = !want.cigars, locate = want.end || want.start, span = want.start != nullptr, resident = b.resident;
    int64_t b_len_total = b.buf_len;
    const auto t_entry = std::chrono::steady_clock::now();
    if (!prm || n_pairs < 0 || !out_score || (!score_only && (!out_ops || !out_ops_off)) || a.buf_len < 0 || b_len_total < 0) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if (n_pairs > 0 && (!a.start || !a.len || !b.start || !b.len)) { set_err("null window table%s", ""); return GNX_EINVAL; }
    if (locate && (!score_only || !want.end)) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if (locate && prm->mode != GNX_AFFINE_GAP_LOCAL) { set_err("gnx_locate_*: the mode must be GNX_AFFINE_GAP_LOCAL%s", ""); return GNX_EINVAL; }
    Ctx &c0 = ctx_at(0);
    int rc;
    { CtxScope sc(c0); if ((rc = ensure_init())) return rc; }
    g_transport = 0; g_bcast_ms = 0;
    if (resident) {
        if (c0.ref_len < 0) { set_err("no resident reference: call gnx_set_reference first%s", ""); return GNX_EINVAL; }
        b_len_total = c0.ref_len;
    }
    long double sum_b = 0;
    for (int64_t p = 0; p < n_pairs; p++) {
        if (a.start[p] < 0 || a.len[p] < 0 || a.start[p] + a.len[p] > a.buf_len || b.start[p] < 0 || b.len[p] < 0 || b.start[p] + b.len[p] > b_len_total) {
            set_err("window out of bounds at pair %s%lld", "", (long long)p); return GNX_EINVAL;
        }
        sum_b += (long double)b.len[p];
    }
    const int nc = std::max(1, std::min<int>(g_nctx, (int)std::max<int64_t>(n_pairs / 8, 1)));
    const std::vector<int64_t> bounds = partition_by_cells(a.len, b.len, n_pairs, nc);
    // a beta buffer that the pairs share (one chunk for every read; windows that overlap) goes to the devices whole -- once to
    // device 0, from there over RCCL; disjoint windows (one per pair) travel with their sub-batches instead
    const bool whole_b = !resident && b_len_total > 0 && (sum_b > 1.5L * (long double)b_len_total || b_len_total <= ((int64_t)16 << 20));
    std::vector<void *> bdev((size_t)nc, nullptr);
    if (resident) {
        if ((rc = ensure_reference(nc))) return rc;
        for (int d = 0; d < nc; d++) {
            bdev[(size_t)d] = ctx_at(d).ref.p;
            if (!bdev[(size_t)d] && b_len_total > 0) { set_err("context %s%lld has no resident reference", "", (long long)d); return GNX_EINVAL; }
        }
    } else if (whole_b) {
        for (int d = 0; d < nc; d++) {
            Ctx &c = ctx_at(d);
            CtxScope sc(c);
            if ((rc = ensure_init())) return rc;
            if ((rc = c.in_b.ensure((size_t)b_len_total + 16))) return rc;
            bdev[(size_t)d] = c.in_b.p;
        }
        { CtxScope sc(c0); HIPCHK(hipSetDevice(c0.device)); HIPCHK(hipMemcpy(c0.in_b.p, b.buf, (size_t)b_len_total, hipMemcpyHostToDevice)); }
        if ((rc = broadcast_from_ctx0(c0.in_b.p, bdev, (size_t)b_len_total))) return rc;
    }
    std::vector<HostJob> jobs((size_t)nc);
    for (int d = 0; d < nc; d++) {
        HostJob &j = jobs[(size_t)d];
        j.c = &ctx_at(d); j.prm = prm; j.p0 = bounds[(size_t)d]; j.p1 = bounds[(size_t)d + 1];
        j.a = a; j.b = b; j.want = want;
        j.b_dev = (const uint8_t *)bdev[(size_t)d];
        j.packed = resident;
    }
    auto work = [](HostJob *j) {
        CtxScope sc(*j->c);
        g_err[0] = 0;
        j->rc = ensure_init();
        if (!j->rc) j->rc = run_host_job(*j);
        if (j->rc) memcpy(j->err, g_err, sizeof(j->err));
    };
    std::vector<std::thread> th;
    for (int d = 1; d < nc; d++) th.emplace_back(work, &jobs[(size_t)d]);
    work(&jobs[0]);
    for (auto &t : th) t.join();
    for (int d = 0; d < nc; d++) if (jobs[(size_t)d].rc) { memcpy(g_err, jobs[(size_t)d].err, sizeof(g_err)); publish_err(); return jobs[(size_t)d].rc; }
    int64_t total = 0;
    for (int d = 0; d < nc; d++) total += jobs[(size_t)d].total_ops;
    // ---- gather on device 0 (input order == context order), then one D2H into pinned result arrays ----
    const auto t_fetch = std::chrono::steady_clock::now();
    gnx_cigar *ops = (gnx_cigar *)g_pool.get((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_cigar));
    int64_t *off = (int64_t *)g_pool.get((size_t)(n_pairs + 1) * 8);
    if (!ops || !off) { if (ops) g_pool.put(ops); if (off) g_pool.put(off); set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
    auto fail = [&](int code) { g_pool.put(ops); g_pool.put(off); return code; };
    CtxScope sc(c0);
    if (hipSetDevice(c0.device) != hipSuccess) { set_err("hipSetDevice failed%s", ""); return fail(GNX_EDEVICE); }
    double gather_ms = 0;
    const int64_t *d_score = (const int64_t *)c0.res_score.p, *d_off = (const int64_t *)c0.res_off.p;
    const gnx_cigar *d_ops = (const gnx_cigar *)c0.res_ops.p;
    if (nc > 1) {
        if ((rc = c0.gat_score.ensure((size_t)std::max<int64_t>(n_pairs, 1) * 8))) return fail(rc);
        if ((rc = c0.gat_off.ensure((size_t)(n_pairs + nc) * 8))) return fail(rc);
        if ((rc = c0.gat_ops.ensure((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_cigar)))) return fail(rc);
        if (locate && (rc = c0.gat_end.ensure((size_t)std::max<int64_t>(n_pairs, 1) * 8))) return fail(rc);
        if (span && (rc = c0.gat_start.ensure((size_t)std::max<int64_t>(n_pairs, 1) * 8))) return fail(rc);
        // context 0's own share never goes through RCCL (no send-to-self): a device-to-device copy on its stream
        auto gather_local = [&]() -> int {
            HostJob &j = jobs[0];
            const int64_t nd = j.p1 - j.p0;
            HIPCHK(hipSetDevice(c0.device));
            if (nd > 0) {
                HIPCHK(hipMemcpyAsync((int64_t *)c0.gat_score.p + j.p0, c0.res_score.p, (size_t)nd * 8, hipMemcpyDeviceToDevice, c0.own_stream));
                HIPCHK(hipMemcpyAsync((int64_t *)c0.gat_off.p + j.p0, c0.res_off.p, (size_t)(nd + 1) * 8, hipMemcpyDeviceToDevice, c0.own_stream));
                if (locate) HIPCHK(hipMemcpyAsync((int64_t *)c0.gat_end.p + j.p0, c0.res_end.p, (size_t)nd * 8, hipMemcpyDeviceToDevice, c0.own_stream));
                if (span) HIPCHK(hipMemcpyAsync((int64_t *)c0.gat_start.p + j.p0, c0.res_start.p, (size_t)nd * 8, hipMemcpyDeviceToDevice, c0.own_stream));
            }
            if (j.total_ops > 0) HIPCHK(hipMemcpyAsync(c0.gat_ops.p, c0.res_ops.p, (size_t)j.total_ops * sizeof(gnx_cigar), hipMemcpyDeviceToDevice, c0.own_stream));
            return GNX_OK;
        };
        auto gather_rccl = [&]() -> int {
            int64_t obase = jobs[0].total_ops;
            const int grc = rccl_grouped([&]() -> int {
                for (int d = 1; d < nc; d++) {
                    HostJob &j = jobs[(size_t)d];
                    Ctx &c = *j.c;
                    const int64_t nd = j.p1 - j.p0;
                    HIPCHK(hipSetDevice(c.device));
                    if (nd > 0) {
                        RCCLCHK(g_rccl.Send(c.res_score.p, (size_t)nd, ncclInt64, 0, g_rccl.comms[(size_t)d], c.own_stream));
                        RCCLCHK(g_rccl.Send(c.res_off.p, (size_t)nd + 1, ncclInt64, 0, g_rccl.comms[(size_t)d], c.own_stream));
                        if (locate) RCCLCHK(g_rccl.Send(c.res_end.p, (size_t)nd, ncclInt64, 0, g_rccl.comms[(size_t)d], c.own_stream));
                        if (span) RCCLCHK(g_rccl.Send(c.res_start.p, (size_t)nd, ncclInt64, 0, g_rccl.comms[(size_t)d], c.own_stream));
                    }
                    if (d == 1 && rccl_injected_failure(2)) return GNX_EDEVICE; // (a send is enqueued, its receive is not)
                    if (j.total_ops > 0) RCCLCHK(g_rccl.Send(c.res_ops.p, (size_t)j.total_ops * 2, ncclInt64, 0, g_rccl.comms[(size_t)d], c.own_stream));
                    HIPCHK(hipSetDevice(c0.device));
                    if (nd > 0) {
                        RCCLCHK(g_rccl.Recv((int64_t *)c0.gat_score.p + j.p0, (size_t)nd, ncclInt64, d, g_rccl.comms[0], c0.own_stream));
                        RCCLCHK(g_rccl.Recv((int64_t *)c0.gat_off.p + j.p0 + d, (size_t)nd + 1, ncclInt64, d, g_rccl.comms[0], c0.own_stream));
                        if (locate) RCCLCHK(g_rccl.Recv((int64_t *)c0.gat_end.p + j.p0, (size_t)nd, ncclInt64, d, g_rccl.comms[0], c0.own_stream));
                        if (span) RCCLCHK(g_rccl.Recv((int64_t *)c0.gat_start.p + j.p0, (size_t)nd, ncclInt64, d, g_rccl.comms[0], c0.own_stream));
                    }
                    if (j.total_ops > 0) RCCLCHK(g_rccl.Recv((gnx_cigar *)c0.gat_ops.p + obase, (size_t)j.total_ops * 2, ncclInt64, d, g_rccl.comms[0], c0.own_stream));
                    obase += j.total_ops;
                }
                return GNX_OK;
            });
            if (grc) return grc;
            for (int d = 0; d < nc; d++) { Ctx &c = *jobs[(size_t)d].c; HIPCHK(hipSetDevice(c.device)); HIPCHK(hipStreamSynchronize(c.own_stream)); }
            HIPCHK(hipSetDevice(c0.device));
            return GNX_OK;
        };
        auto gather_copies = [&]() -> int {
            int64_t obase = jobs[0].total_ops;
            for (int d = 1; d < nc; d++) {
                HostJob &j = jobs[(size_t)d];
                Ctx &c = *j.c;
                const int64_t nd = j.p1 - j.p0;
                if (nd > 0) {
                    HIPCHK(hipMemcpyPeer((int64_t *)c0.gat_score.p + j.p0, c0.device, c.res_score.p, c.device, (size_t)nd * 8));
                    HIPCHK(hipMemcpyPeer((int64_t *)c0.gat_off.p + j.p0 + d, c0.device, c.res_off.p, c.device, (size_t)(nd + 1) * 8));
                    if (locate) HIPCHK(hipMemcpyPeer((int64_t *)c0.gat_end.p + j.p0, c0.device, c.res_end.p, c.device, (size_t)nd * 8));
                    if (span) HIPCHK(hipMemcpyPeer((int64_t *)c0.gat_start.p + j.p0, c0.device, c.res_start.p, c.device, (size_t)nd * 8));
                }
                if (j.total_ops > 0) HIPCHK(hipMemcpyPeer((gnx_cigar *)c0.gat_ops.p + obase, c0.device, c.res_ops.p, c.device, (size_t)j.total_ops * sizeof(gnx_cigar)));
                obase += j.total_ops;
            }
            HIPCHK(hipSetDevice(c0.device));
            return GNX_OK;
        };
        auto gather = [&]() -> int {
            int r = gather_local();
            if (r) return r;
            // every rank of the communicator must take part in a grouped exchange: only when the call uses all contexts
            bool via_rccl = rccl_active() && (int)g_rccl.comms.size() == nc;
            if (via_rccl && gather_rccl() != GNX_OK) { rccl_give_up(); via_rccl = false; if ((r = gather_local())) return r; }
            if (!via_rccl && (r = gather_copies())) return r;
            HIPCHK(hipStreamSynchronize(c0.own_stream));
            g_transport = via_rccl ? 1 : (g_rccl_broken ? 3 : 2);
            return GNX_OK;
        };
        const auto t_gather = std::chrono::steady_clock::now();
        if ((rc = gather())) return fail(rc);
        gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_gather).count();
        d_score = (const int64_t *)c0.gat_score.p; d_ops = (const gnx_cigar *)c0.gat_ops.p;
    }
    auto fetch = [&]() -> int {
        hipStream_t st = c0.own_stream;
        if (n_pairs) HIPCHK(hipMemcpyAsync(out_score, d_score, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
        if (n_pairs && locate) HIPCHK(hipMemcpyAsync(want.end, nc > 1 ? c0.gat_end.p : c0.res_end.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
        if (n_pairs && span) HIPCHK(hipMemcpyAsync(want.start, nc > 1 ? c0.gat_start.p : c0.res_start.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
        if (total) HIPCHK(hipMemcpyAsync(ops, d_ops, (size_t)total * sizeof(gnx_cigar), hipMemcpyDeviceToHost, st));
        if (score_only) { /* only the score vector comes back */ }
        else if (nc == 1) HIPCHK(hipMemcpyAsync(off, d_off, (size_t)(n_pairs + 1) * 8, hipMemcpyDeviceToHost, st));
        else {
            // each context's offsets (n_d + 1 of them, starting at 0) sit at [p0 + d ..]: rebase on the host while copying
            std::vector<int64_t> tmp((size_t)(n_pairs + nc));
            HIPCHK(hipMemcpyAsync(tmp.data(), c0.gat_off.p, (size_t)(n_pairs + nc) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            int64_t base = 0;
            for (int d = 0; d < nc; d++) {
                const HostJob &j = jobs[(size_t)d];
                for (int64_t q = j.p0; q < j.p1; q++) off[q] = tmp[(size_t)(q + d)] + base;
                base += j.total_ops;
            }
            off[n_pairs] = base;
        }
        HIPCHK(hipStreamSynchronize(st));
        return GNX_OK;
    };
    if ((rc = fetch())) return fail(rc);
    // per-call timing = the slowest context (they run side by side); cells and bytes add up
    gnx_timing t = jobs[0].timing;
    for (int d = 1; d < nc; d++) {
        const gnx_timing &u = jobs[(size_t)d].timing;
        t.fill_ms = std::max(t.fill_ms, u.fill_ms); t.traceback_ms = std::max(t.traceback_ms, u.traceback_ms); t.total_ms = std::max(t.total_ms, u.total_ms);
        if (score_only) t.fast_path = std::max(t.fast_path, u.fast_path);
        t.dominant_ms = std::max(t.dominant_ms, u.dominant_ms); t.cells += u.cells; t.trace_bytes += u.trace_bytes; t.n_launches += u.n_launches; t.dominant_launches += u.dominant_launches;
    }
    t.fetch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fetch).count();
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    t.transport = g_transport; t.n_contexts = nc; t.gather_ms = gather_ms; t.bcast_ms = g_bcast_ms;
    c0.timing = t;
    if (getenv("GNX_DEBUG")) fprintf(stderr, "[gnx host] %lld pairs on %d context(s): call %.3f ms = first upload %.3f + kernels %.3f (device, slowest context) + gather / D2H %.3f (gather %.3f, transport %d) + broadcast %.3f + rest\n",
                                     (long long)n_pairs, nc, t.host_ms, t.stage0_ms, t.total_ms, t.fetch_ms, t.gather_ms, t.transport, t.bcast_ms);
    if (score_only) { g_pool.put(ops); g_pool.put(off); return GNX_OK; }
    *out_ops = ops; *out_ops_off = off;
    return GNX_OK;
}

// ---- gnx_best_of_*: reads x candidate windows x strands -> per read the first best candidate and its CIGAR (gnx_align.h) ----------
// One context (context 0).  The reads go up once; their reverse complements are written behind them on the device, so a candidate's
// read is a window (start, len) of that buffer like any other alpha window, and both stages run the twins' own device drivers:
//   score stage   score_or_fallback over the candidates, in sub-batches of GNX_HOST_SUB pairs (a read's candidates may straddle a cut)
//   selection     first_max_kernel; only best[] (4 bytes per read) comes back: the host plans the CIGAR stage from the winners' lengths
//   CIGAR stage   winner_tables_kernel builds the winners' start tables from what is resident, run_device aligns them in sub-batches
// Nothing is written to the caller's outputs before both stages have succeeded.
// gnx_best_pair_* (pr != nullptr) is the same body: its score stage also asks for every candidate's target start, pair_select_kernel
// stands where first_max_kernel stands, and a few more vectors come back.
enum { BO_READS, BO_ROFF, BO_COFF, BO_WREAD, BO_RS, BO_WS, BO_CSCORE, BO_CEND, BO_BEST, BO_BSCORE, BO_BEND, BO_WR, BO_WW,
       BO_CSTART, BO_STRAND, BO_BSTART, BO_SECOND, BO_PROPER, BO_TLEN, BO_COUNT };
struct PairOut { // what gnx_best_pair_* has beyond gnx_best_of_*
    const gnx_pair_opts *o;
    int64_t *start, *second; // per read
    uint8_t *proper;         // per pair
    int64_t *tlen;
    int64_t *cand_start, *cand_end; // per candidate (may be null)
};
static_assert(BO_COUNT == sizeof(Ctx::bo) / sizeof(DevBuf), "Ctx::bo holds one buffer per BO_* index");
int run_best_of(const gnx_params *prm, int64_t n_reads, const uint8_t *read_cat, const int64_t *read_off, bool resident, const uint8_t *t_buf, int64_t t_len,
                const int64_t *cand_off, const int64_t *cand_start, const int64_t *cand_len, const uint8_t *cand_strand,
                int32_t *out_best, int64_t *out_score, int64_t *out_end, int64_t *out_cand_score, gnx_cigar **out_ops, int64_t **out_ops_off,
                const PairOut *pr = nullptr) {
    const auto t_entry = std::chrono::steady_clock::now();
    // ---- argument checks: everything that needs no device ----
    if (!prm || n_reads < 0 || !read_off || !cand_off || !out_best || !out_score || t_len < 0) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if ((out_ops == nullptr) != (out_ops_off == nullptr)) { set_err("out_ops and out_ops_off must be given together%s", ""); return GNX_EINVAL; }
    if (prm->mode < GNX_AFFINE_GAP || prm->mode > GNX_CONST_GAP_HIGHMEM) { set_err("unknown mode %s%lld", "", (long long)prm->mode); return GNX_EINVAL; }
    const bool local = prm->mode == GNX_AFFINE_GAP_LOCAL, cigars = out_ops != nullptr;
    if (out_end && !local) { set_err("out_target_end is defined for GNX_AFFINE_GAP_LOCAL only%s", ""); return GNX_EINVAL; }
    if (pr) {
        if (!pr->o || !out_end || !pr->start || !pr->proper || !pr->tlen) { set_err("bad argument%s", ""); return GNX_EINVAL; }
        if (!local) { set_err("gnx_best_pair_*: the mode must be GNX_AFFINE_GAP_LOCAL%s", ""); return GNX_EINVAL; }
        if (n_reads & 1) { set_err("gnx_best_pair_*: n_reads must be even (reads 2k and 2k + 1 are mates)%s", ""); return GNX_EINVAL; }
        if (pr->o->min_insert < 0 || pr->o->max_insert < pr->o->min_insert || pr->o->unpaired_penalty < 0) { set_err("gnx_best_pair_*: 0 <= min_insert <= max_insert and unpaired_penalty >= 0%s", ""); return GNX_EINVAL; }
    }
    if (read_off[0] < 0 || cand_off[0] != 0) { set_err("read_off must start at >= 0 and cand_off at 0%s", ""); return GNX_EINVAL; }
    for (int64_t r = 0; r < n_reads; r++)
        if (read_off[r + 1] < read_off[r] || cand_off[r + 1] < cand_off[r]) { set_err("decreasing offsets at read %s%lld", "", (long long)r); return GNX_EINVAL; }
    const int64_t n_cand = cand_off[n_reads], r_lo = read_off[0], r_total = read_off[n_reads] - r_lo;
    if ((n_cand > 0 && (!cand_start || !cand_len || !cand_strand)) || (r_total > 0 && !read_cat) || (!resident && t_len > 0 && !t_buf)) { set_err("null table or buffer%s", ""); return GNX_EINVAL; }
    for (int64_t q = 0; q < n_cand; q++) {
        if (cand_strand[q] > 1) { set_err("strand byte > 1 at candidate %s%lld", "", (long long)q); return GNX_EINVAL; }
        if (cand_start[q] < 0 || cand_len[q] < 0 || (!resident && cand_len[q] > t_len - cand_start[q])) { set_err("window out of bounds at candidate %s%lld", "", (long long)q); return GNX_EINVAL; }
    }
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    if (resident) {
        if (c.ref_len < 0) { set_err("no resident reference: call gnx_set_reference first%s", ""); return GNX_EINVAL; }
        for (int64_t q = 0; q < n_cand; q++)
            if (cand_len[q] > c.ref_len - cand_start[q]) { set_err("window out of bounds at candidate %s%lld", "", (long long)q); return GNX_EINVAL; }
    }
    hipStream_t st = c.own_stream;
    const int64_t sub = gnx_host_sub(getenv("GNX_HOST_SUB"));

    // ---- host tables: per candidate its read as a window of [reads | reverse complements]; the reads that have candidates ----
    std::vector<int64_t> h_rs((size_t)n_cand), h_rlen((size_t)n_cand), win_read;
    for (int64_t r = 0; r < n_reads; r++) {
        for (int64_t q = cand_off[r]; q < cand_off[r + 1]; q++) { h_rs[(size_t)q] = read_off[r] - r_lo + (cand_strand[q] ? r_total : 0); h_rlen[(size_t)q] = read_off[r + 1] - read_off[r]; }
        if (cigars && cand_off[r + 1] > cand_off[r]) win_read.push_back(r);
    }
    const int64_t n_win = (int64_t)win_read.size();
    std::vector<int64_t> h_roff;
    if (r_lo) { h_roff.resize((size_t)n_reads + 1); for (int64_t r = 0; r <= n_reads; r++) h_roff[(size_t)r] = read_off[r] - r_lo; }

    // ---- uploads: the reads once, 16 bytes of table per candidate, the offsets ----
    DevBuf *bo = c.bo;
    const size_t nr = (size_t)std::max<int64_t>(n_reads, 1), ncd = (size_t)std::max<int64_t>(n_cand, 1);
    if ((rc = bo[BO_READS].ensure((size_t)r_total * 2 + 16)) || (rc = bo[BO_ROFF].ensure((nr + 1) * 8)) || (rc = bo[BO_COFF].ensure((nr + 1) * 8)) ||
        (rc = bo[BO_RS].ensure(ncd * 8)) || (rc = bo[BO_WS].ensure(ncd * 8)) || (rc = bo[BO_CSCORE].ensure(ncd * 8)) || (local && (rc = bo[BO_CEND].ensure(ncd * 8))) ||
        (rc = bo[BO_BEST].ensure(nr * 4)) || (rc = bo[BO_BSCORE].ensure(nr * 8)) || (rc = bo[BO_BEND].ensure(nr * 8))) return rc;
    if (pr && ((rc = bo[BO_CSTART].ensure(ncd * 8)) || (rc = bo[BO_STRAND].ensure(ncd)) || (rc = bo[BO_BSTART].ensure(nr * 8)) || (rc = bo[BO_SECOND].ensure(nr * 8)) ||
               (rc = bo[BO_PROPER].ensure(nr)) || (rc = bo[BO_TLEN].ensure(nr * 8)))) return rc;
    if (!resident && (rc = c.in_b.ensure((size_t)t_len + 16))) return rc;
    uint8_t *d_reads = (uint8_t *)bo[BO_READS].p;
    const uint8_t *d_tbuf = resident ? (const uint8_t *)c.ref.p : (const uint8_t *)c.in_b.p;
    int64_t *d_rs = (int64_t *)bo[BO_RS].p, *d_ws = (int64_t *)bo[BO_WS].p, *d_cscore = (int64_t *)bo[BO_CSCORE].p, *d_cend = local ? (int64_t *)bo[BO_CEND].p : nullptr;
    int64_t *d_cstart = pr ? (int64_t *)bo[BO_CSTART].p : nullptr;
    if (n_reads > 0 && n_cand > 0) {
        if (r_total) HIPCHK(hipMemcpyAsync(d_reads, read_cat + r_lo, (size_t)r_total, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(bo[BO_ROFF].p, r_lo ? h_roff.data() : read_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(bo[BO_COFF].p, cand_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_rs, h_rs.data(), (size_t)n_cand * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ws, cand_start, (size_t)n_cand * 8, hipMemcpyHostToDevice, st));
        if (pr) HIPCHK(hipMemcpyAsync(bo[BO_STRAND].p, cand_strand, (size_t)n_cand, hipMemcpyHostToDevice, st));
        if (!resident && t_len) HIPCHK(hipMemcpyAsync(c.in_b.p, t_buf, (size_t)t_len, hipMemcpyHostToDevice, st));
        if (r_total) {
            hipLaunchKernelGGL(revcomp_reads_kernel, dim3((unsigned)std::min<int64_t>((n_reads + 3) / 4, 1 << 20)), dim3(256), 0, st, (const uint8_t *)d_reads, (const int64_t *)bo[BO_ROFF].p, n_reads, d_reads + r_total);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(st)); // (the sources are pageable memory of the caller and locals of this call: no return while a copy may still read them)
    }
    // ---- score stage ----
    gnx_timing tsum = {};
    if (n_cand > 0) {
        const int64_t size = sub_batch_size(n_cand, sub);
        for (int64_t b = 0; b < n_cand; b += size) {
            const int64_t cnt = std::min(size, n_cand - b);
            const int64_t *h_rl = h_rlen.data() + b, *h_wl = cand_len + b;
            int64_t *d_st = d_cstart ? d_cstart + b : nullptr;
            if (!local) { // alpha = the read or its reverse complement, beta = the window
                PackedBeta pb(c, resident);
                rc = score_or_fallback(c, prm, cnt, d_reads, d_rs + b, d_tbuf, d_ws + b, h_rl, h_wl, d_cscore + b, st);
            } else if (!resident) // target (alpha) = the window, query (beta) = the read
                rc = score_or_fallback(c, prm, cnt, d_tbuf, d_ws + b, d_reads, d_rs + b, h_wl, h_rl, d_cscore + b, st, d_cend + b, true, d_st);
            else // the local sweep reads its target packed (the kernels' beta); only its fallback needs bytes
                rc = locate_reads_in_windows(c, prm, cnt, d_reads, d_rs + b, h_rl, d_tbuf, d_ws + b, h_wl, true, d_cscore + b, d_cend + b, d_st, st);
            if (rc) return rc;
            add_timing(tsum, c.timing, true);
        }
        if (pr) {
            PairSelectArgs pa{d_cscore, d_cstart, d_cend, d_ws, (const int64_t *)bo[BO_COFF].p, (const uint8_t *)bo[BO_STRAND].p, n_reads / 2, pr->o->min_insert, pr->o->max_insert,
                              pr->o->unpaired_penalty, (int32_t *)bo[BO_BEST].p, (int64_t *)bo[BO_BSCORE].p, (int64_t *)bo[BO_BSTART].p, (int64_t *)bo[BO_BEND].p,
                              (int64_t *)bo[BO_SECOND].p, (uint8_t *)bo[BO_PROPER].p, (int64_t *)bo[BO_TLEN].p};
            hipLaunchKernelGGL(pair_select_kernel, dim3((unsigned)std::min<int64_t>(n_reads / 2, 1 << 20)), dim3(64), 0, st, pa);
        } else
            hipLaunchKernelGGL(first_max_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, (const int64_t *)d_cscore, (const int64_t *)d_cend, (const int64_t *)bo[BO_COFF].p,
                               n_reads, (int32_t *)bo[BO_BEST].p, (int64_t *)bo[BO_BSCORE].p, (int64_t *)bo[BO_BEND].p);
        HIPCHK(hipGetLastError());
    }

    // ---- CIGAR stage: the winners only ----
    std::vector<int32_t> h_best((size_t)n_reads, -1);
    int64_t total = 0;
    if (n_win > 0) {
        if ((rc = bo[BO_WREAD].ensure((size_t)n_win * 8)) || (rc = bo[BO_WR].ensure((size_t)n_win * 8)) || (rc = bo[BO_WW].ensure((size_t)n_win * 8)) ||
            (rc = c.res_score.ensure((size_t)n_win * 8)) || (rc = c.res_off.ensure((size_t)(n_win + 1) * 8))) return rc;
        int64_t *d_wr = (int64_t *)bo[BO_WR].p, *d_ww = (int64_t *)bo[BO_WW].p;
        HIPCHK(hipMemcpyAsync(bo[BO_WREAD].p, win_read.data(), (size_t)n_win * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(winner_tables_kernel, dim3((unsigned)((n_win + 255) / 256)), dim3(256), 0, st, (const int32_t *)bo[BO_BEST].p, (const int64_t *)bo[BO_COFF].p,
                           (const int64_t *)bo[BO_WREAD].p, (const int64_t *)d_rs, (const int64_t *)d_ws, n_win, d_wr, d_ww);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_best.data(), bo[BO_BEST].p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st)); // all that crosses between the stages
        HIPCHK(hipStreamSynchronize(st));
        std::vector<int64_t> w_rlen((size_t)n_win), w_wlen((size_t)n_win);
        int64_t worst = 0;
        for (int64_t w = 0; w < n_win; w++) {
            const int64_t r = win_read[(size_t)w];
            w_rlen[(size_t)w] = read_off[r + 1] - read_off[r]; w_wlen[(size_t)w] = cand_len[cand_off[r] + h_best[(size_t)r]];
            worst += w_rlen[(size_t)w] + w_wlen[(size_t)w] + 1;
        }
        const int64_t size = sub_batch_size(n_win, sub);
        if ((rc = grow_ops(c, 0, std::max<int64_t>(std::min<int64_t>(worst, std::max<int64_t>((int64_t)1 << 20, 64 * std::min(n_win, size))), 1), st))) return rc;
        gnx_timing tal = {};
        for (int64_t b = 0; b < n_win; b += size) {
            const int64_t cnt = std::min(size, n_win - b);
            const int64_t *h_rl = w_rlen.data() + b, *h_wl = w_wlen.data() + b;
            if (local && resident && (rc = unpack_ref_windows(c, d_ww + b, h_wl, cnt, st))) return rc; // only the winners' windows
            PackedBeta pb(c, !local && resident);
            rc = run_sub_batch_cigars(c, n_win, b, cnt, total, st, [&](int64_t *d_sc, gnx_cigar *d_ops, int64_t cap, int64_t *d_off, int64_t *tot) {
                if (!local) return run_device(prm, cnt, d_reads, d_wr + b, d_tbuf, d_ww + b, h_rl, h_wl, d_sc, d_ops, cap, d_off, tot, st);
                if (resident) return run_device(prm, cnt, (const uint8_t *)c.in_b.p, (const int64_t *)c.in_bl.p, d_reads, d_wr + b, h_wl, h_rl, d_sc, d_ops, cap, d_off, tot, st);
                return run_device(prm, cnt, d_tbuf, d_ww + b, d_reads, d_wr + b, h_wl, h_rl, d_sc, d_ops, cap, d_off, tot, st);
            });
            if (rc) return rc;
            tal.total_ms += c.timing.total_ms;
        }
        tsum.total_ms += tal.total_ms;
    }

    // ---- results: pinned CIGAR arrays (gnx_free), the rest into the caller's arrays ----
    const auto t_fetch = std::chrono::steady_clock::now();
    gnx_cigar *ops = nullptr;
    int64_t *off = nullptr;
    if (cigars) {
        ops = (gnx_cigar *)g_pool.get((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_cigar));
        off = (int64_t *)g_pool.get((size_t)(n_reads + 1) * 8);
        if (!ops || !off) { if (ops) g_pool.put(ops); if (off) g_pool.put(off); set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
    }
    std::vector<int64_t> w_score((size_t)n_win), w_off((size_t)n_win + 1, 0), h_bscore((size_t)n_reads, 0), h_bend((size_t)n_reads, 0), h_cscore(out_cand_score ? (size_t)n_cand : 0);
    const int64_t n_mates = n_reads / 2;
    std::vector<int64_t> h_bstart(pr ? (size_t)n_reads : 0, 0), h_second(pr ? (size_t)n_reads : 0, INT64_MIN), h_tlen(pr ? (size_t)n_mates : 0, 0),
        h_cstart(pr && pr->cand_start ? (size_t)n_cand : 0), h_cend(pr && pr->cand_end ? (size_t)n_cand : 0);
    std::vector<uint8_t> h_proper(pr ? (size_t)n_mates : 0, 0);
    auto fetch = [&]() -> int {
        if (n_cand > 0 && n_reads > 0) {
            if (!n_win) HIPCHK(hipMemcpyAsync(h_best.data(), bo[BO_BEST].p, (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_bscore.data(), bo[BO_BSCORE].p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
            if (out_end) HIPCHK(hipMemcpyAsync(h_bend.data(), bo[BO_BEND].p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
            if (out_cand_score) HIPCHK(hipMemcpyAsync(h_cscore.data(), d_cscore, (size_t)n_cand * 8, hipMemcpyDeviceToHost, st));
            if (pr) {
                HIPCHK(hipMemcpyAsync(h_bstart.data(), bo[BO_BSTART].p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(h_second.data(), bo[BO_SECOND].p, (size_t)n_reads * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(h_proper.data(), bo[BO_PROPER].p, (size_t)n_mates, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(h_tlen.data(), bo[BO_TLEN].p, (size_t)n_mates * 8, hipMemcpyDeviceToHost, st));
                if (pr->cand_start) HIPCHK(hipMemcpyAsync(h_cstart.data(), d_cstart, (size_t)n_cand * 8, hipMemcpyDeviceToHost, st));
                if (pr->cand_end) HIPCHK(hipMemcpyAsync(h_cend.data(), d_cend, (size_t)n_cand * 8, hipMemcpyDeviceToHost, st));
            }
        }
        if (n_win) {
            HIPCHK(hipMemcpyAsync(w_score.data(), c.res_score.p, (size_t)n_win * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(w_off.data(), c.res_off.p, (size_t)(n_win + 1) * 8, hipMemcpyDeviceToHost, st));
            if (total) HIPCHK(hipMemcpyAsync(ops, c.res_ops.p, (size_t)total * sizeof(gnx_cigar), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return GNX_OK;
    };
    if ((rc = fetch())) { if (ops) g_pool.put(ops); if (off) g_pool.put(off); return rc; }
    for (int64_t r = 0; r < n_reads; r++) { out_best[r] = h_best[(size_t)r]; out_score[r] = h_bscore[(size_t)r]; if (out_end) out_end[r] = h_bend[(size_t)r]; }
    if (out_cand_score && n_cand > 0) memcpy(out_cand_score, h_cscore.data(), (size_t)n_cand * 8);
    if (pr) {
        for (int64_t r = 0; r < n_reads; r++) { pr->start[r] = h_bstart[(size_t)r]; if (pr->second) pr->second[r] = h_second[(size_t)r]; }
        for (int64_t k = 0; k < n_mates; k++) { pr->proper[k] = h_proper[(size_t)k]; pr->tlen[k] = h_tlen[(size_t)k]; }
        if (pr->cand_start && n_cand > 0) memcpy(pr->cand_start, h_cstart.data(), (size_t)n_cand * 8);
        if (pr->cand_end && n_cand > 0) memcpy(pr->cand_end, h_cend.data(), (size_t)n_cand * 8);
    }
    if (cigars) { // a read without candidates: an empty CIGAR
        int64_t w = 0;
        for (int64_t r = 0; r < n_reads; r++) {
            off[r] = w_off[(size_t)w];
            if (w < n_win && win_read[(size_t)w] == r) { out_score[r] = w_score[(size_t)w]; w++; }
        }
        off[n_reads] = total;
        *out_ops = ops; *out_ops_off = off;
    }
    tsum.fetch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fetch).count();
    tsum.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    tsum.n_contexts = 1;
    c.timing = tsum;
    return GNX_OK;
}

// ---- gnx_summarize_*: CIGARs walked against their sequences (aln_summary.hip.h; contract: gnx_align.h) ----------------------------
// One context (context 0).  Everything the host can check is checked before the device is touched: the tables, the windows, and
// every CIGAR run (op, run length, consumption).  Sequences, tables and runs go up once; the summary kernel is launched per
// sub-batch of GNX_HOST_SUB pairs (GNX_SUMMARY_SUB=<pairs> overrides the cut), and with an extended CIGAR asked for the scan
// family chains the sub-batches' offsets through its carry and the WRITE instantiation follows.  Nothing is written to the
// caller's outputs before every kernel has succeeded.
enum { SM_A, SM_B, SM_AS, SM_AL, SM_BS, SM_BL, SM_OPS, SM_OFF, SM_SC, SM_OUT, SM_NX, SM_XOFF, SM_XOPS, SM_MISC, SM_COUNT };
static_assert(SM_COUNT == sizeof(Ctx::sm) / sizeof(DevBuf), "Ctx::sm holds one buffer per SM_* index");
// The argument checks gnx_summarize_* and gnx_md_* share: everything that needs no device.  outs_given: the entry's required outputs are
// there; xops_paired: gnx_summarize_*'s optional pair of outputs comes together or not at all.  cells = the columns of all CIGARs.
int check_cigar_call(const gnx_params *prm, int64_t n_pairs, const SeqSide &sa, const SeqSide &sb, const gnx_cigar *ops, const int64_t *ops_off,
                     bool outs_given, bool xops_paired, int64_t &cells) {
    if (!prm || n_pairs < 0 || !ops_off || !outs_given || !sa.start || !sa.len || !sb.start || !sb.len || sa.buf_len < 0 || sb.buf_len < 0) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if (!xops_paired) { set_err("out_xops and out_xops_off must be given together%s", ""); return GNX_EINVAL; }
    if (prm->mode < GNX_AFFINE_GAP || prm->mode > GNX_CONST_GAP_HIGHMEM) { set_err("unknown mode %s%lld", "", (long long)prm->mode); return GNX_EINVAL; }
    if (ops_off[0] != 0) { set_err("ops_off must start at 0%s", ""); return GNX_EINVAL; }
    for (int64_t q = 0; q < n_pairs; q++)
        if (ops_off[q + 1] < ops_off[q]) { set_err("decreasing ops_off at pair %s%lld", "", (long long)q); return GNX_EINVAL; }
    const int64_t n_runs = ops_off[n_pairs];
    if (n_runs > 0 && !ops) { set_err("null CIGAR array%s", ""); return GNX_EINVAL; }
    for (const SeqSide *s : {&sa, &sb})
        for (int64_t q = 0; q < n_pairs; q++) {
            if (s->start[q] < 0 || s->len[q] < 0 || (!s->resident && s->len[q] > s->buf_len - s->start[q])) { set_err("window out of bounds at pair %s%lld", "", (long long)q); return GNX_EINVAL; }
            if (!s->resident && s->len[q] > 0 && !s->buf) { set_err("null sequence buffer%s", ""); return GNX_EINVAL; }
            if (s->len[q] >= ((int64_t)1 << 30)) { set_err("a sequence of 2^30 bases or more at pair %s%lld (the limit of the align entries)", "", (long long)q); return GNX_EINVAL; }
        }
    cells = 0;
    for (int64_t q = 0; q < n_pairs; q++) {
        int64_t fa = sa.len[q], fb = sb.len[q]; // what is left of either sequence
        for (int64_t x = ops_off[q]; x < ops_off[q + 1]; x++) {
            const int64_t len = ops[x].run_length;
            const int op = ops[x].op;
            if (op > GNX_COL_D) { set_err("unknown CIGAR op at run %s%lld", "", (long long)x); return GNX_EINVAL; }
            if (len < 0) { set_err("negative run length at run %s%lld", "", (long long)x); return GNX_EINVAL; }
            if ((op != GNX_COL_I && len > fa) || (op != GNX_COL_D && len > fb)) { set_err("the CIGAR of pair %s%lld consumes more than its sequences hold", "", (long long)q); return GNX_EINVAL; }
            if (op != GNX_COL_I) fa -= len;
            if (op != GNX_COL_D) fb -= len;
            cells += len;
        }
    }
    return GNX_OK;
}
// ... and the one that needs the context: the windows of a resident side lie inside the reference
int check_resident_windows(const Ctx &c, int64_t n_pairs, const SeqSide &sa, const SeqSide &sb) {
    if (sa.resident || sb.resident) {
        if (c.ref_len < 0) { set_err("no resident reference: call gnx_set_reference first%s", ""); return GNX_EINVAL; }
        const SeqSide &s = sa.resident ? sa : sb;
        for (int64_t q = 0; q < n_pairs; q++)
            if (s.len[q] > c.ref_len - s.start[q]) { set_err("window out of bounds at pair %s%lld", "", (long long)q); return GNX_EINVAL; }
    }
    return GNX_OK;
}

// What both families send up once per call (n_pairs > 0): sequences, window tables, CIGAR runs and offsets, the score matrix, the zeroed
// flag and carry words; `a` gets every field that does not depend on the sub-batch.  Returns which side the kernels read packed in pk.
int sum_upload(Ctx &c, hipStream_t st, const gnx_params *prm, int64_t n_pairs, const SeqSide &sa, const SeqSide &sb, const gnx_cigar *ops, const int64_t *ops_off,
               SumArgs &a, int &pk) {
    DevBuf *sm = c.sm;
    const size_t np = (size_t)n_pairs;
    const int64_t n_runs = ops_off[n_pairs];
    int rc;
    if ((rc = sm[SM_AS].ensure(np * 8)) || (rc = sm[SM_AL].ensure(np * 8)) || (rc = sm[SM_BS].ensure(np * 8)) || (rc = sm[SM_BL].ensure(np * 8)) ||
        (rc = sm[SM_OPS].ensure((size_t)std::max<int64_t>(n_runs, 1) * sizeof(gnx_cigar))) || (rc = sm[SM_OFF].ensure((np + 1) * 8)) || (rc = sm[SM_SC].ensure(25 * 8)) ||
        (rc = sm[SM_NX].ensure(np * 8)) || (rc = sm[SM_XOFF].ensure((np + 1) * 8)) || (rc = sm[SM_MISC].ensure(64)) ||
        (!sa.resident && (rc = sm[SM_A].ensure((size_t)sa.buf_len + 16))) || (!sb.resident && (rc = sm[SM_B].ensure((size_t)sb.buf_len + 16)))) return rc;
    memset(&a, 0, sizeof(a));
    for (int side = 0; side < 2; side++) {
        const SeqSide &s = side ? sb : sa;
        KParams &k = a.kp;
        if (s.resident) { k.b2 = (const unsigned *)c.ref.p; k.bflag = (const unsigned long long *)c.ref_flag.p; k.brank = (const unsigned *)c.ref_rank.p; k.bexc = (const unsigned long long *)c.ref_exc.p; }
        else if (s.buf_len > 0) HIPCHK(hipMemcpyAsync(sm[side ? SM_B : SM_A].p, s.buf, (size_t)s.buf_len, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(sm[side ? SM_BS : SM_AS].p, s.start, np * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(sm[side ? SM_BL : SM_AL].p, s.len, np * 8, hipMemcpyHostToDevice, st));
    }
    if (n_runs > 0) HIPCHK(hipMemcpyAsync(sm[SM_OPS].p, ops, (size_t)n_runs * sizeof(gnx_cigar), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sm[SM_OFF].p, ops_off, (np + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(sm[SM_SC].p, prm->scores, 25 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(sm[SM_MISC].p, 0, 64, st)); // [0] the error flags (int), [8 ..) the scan's carry (int64)
    a.a_buf = sa.resident ? nullptr : (const uint8_t *)sm[SM_A].p; a.b_buf = sb.resident ? nullptr : (const uint8_t *)sm[SM_B].p;
    a.ops = (const gnx_cigar *)sm[SM_OPS].p; a.scores = (const int64_t *)sm[SM_SC].p;
    a.local = prm->mode == GNX_AFFINE_GAP_LOCAL;
    a.err = (int *)sm[SM_MISC].p;
    pk = sa.resident ? 1 : sb.resident ? 2 : 0;
    return GNX_OK;
}
// `a` for the sub-batch of cnt pairs from pair b: its slices of the per-pair tables
SumArgs sum_sub_args(const SumArgs &a, DevBuf *sm, int64_t b, int64_t cnt) {
    SumArgs s = a;
    s.a_start = (const int64_t *)sm[SM_AS].p + b; s.a_len = (const int64_t *)sm[SM_AL].p + b; s.b_start = (const int64_t *)sm[SM_BS].p + b; s.b_len = (const int64_t *)sm[SM_BL].p + b;
    s.ops_off = (const int64_t *)sm[SM_OFF].p + b; s.out = (gnx_aln_summary *)sm[SM_OUT].p + b; s.nx = (int64_t *)sm[SM_NX].p + b; s.xoff = (const int64_t *)sm[SM_XOFF].p + b;
    s.n_pairs = cnt;
    return s;
}
// GNX_EBASE's check of that sub-batch (aln_summary_bases_kernel): one workgroup per pair, or several that share a pair when the launch is a few long pairs
void launch_sum_bases(SumArgs s, int pk, const SeqSide &sa, const SeqSide &sb, int64_t b, int64_t cnt, hipStream_t st) {
    int64_t longest = 0;
    for (int64_t q = b; q < b + cnt; q++) longest = std::max(longest, std::max(sa.len[q], sb.len[q]));
    const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(longest / 8192, 256), ((int64_t)1 << 16) / cnt));
    const dim3 bgrid((unsigned)std::min<int64_t>(cnt, 1 << 20), (unsigned)chunks);
    s.slice = (int)((((longest + chunks - 1) / chunks) + 255) & ~(int64_t)255) + 256;
    if (pk == 1) hipLaunchKernelGGL(aln_summary_bases_kernel<1>, bgrid, dim3(256), 0, st, s);
    else if (pk == 2) hipLaunchKernelGGL(aln_summary_bases_kernel<2>, bgrid, dim3(256), 0, st, s);
    else hipLaunchKernelGGL(aln_summary_bases_kernel<0>, bgrid, dim3(256), 0, st, s);
}

int run_summarize(const gnx_params *prm, int64_t n_pairs, const SeqSide &sa, const SeqSide &sb, const gnx_cigar *ops, const int64_t *ops_off,
                  gnx_aln_summary *out, gnx_cigar **out_xops, int64_t **out_xops_off) {
    const auto t_entry = std::chrono::steady_clock::now();
    int rc;
    int64_t cells = 0;
    if ((rc = check_cigar_call(prm, n_pairs, sa, sb, ops, ops_off, out != nullptr, (out_xops == nullptr) == (out_xops_off == nullptr), cells))) return rc;
    const bool local = prm->mode == GNX_AFFINE_GAP_LOCAL, affine = local || prm->mode == GNX_AFFINE_GAP || prm->mode == GNX_AFFINE_GAP_HIGHMEM, xc = out_xops != nullptr;
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    if ((rc = check_resident_windows(c, n_pairs, sa, sb))) return rc;
    hipStream_t st = c.own_stream;
    gnx_cigar *xops = nullptr;
    int64_t *xoff = nullptr;
    if (xc) {
        xoff = (int64_t *)g_pool.get((size_t)(n_pairs + 1) * 8);
        if (!xoff) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
        xoff[0] = 0;
    }
    auto fail = [&](int r) { if (xoff) g_pool.put(xoff); if (xops) g_pool.put(xops); return r; };
    gnx_timing t = {};
    t.fast_path = 12; t.cells = cells; t.n_contexts = 1;
    int64_t n_x = 0;
    std::vector<gnx_aln_summary> h_out((size_t)n_pairs);
    if (n_pairs > 0) {
        int64_t sub = gnx_host_sub(getenv("GNX_HOST_SUB"));
        if (const char *e = getenv("GNX_SUMMARY_SUB")) sub = std::max<int64_t>(atoll(e), 1);
        int cut = 64;
        if (const char *e = getenv("GNX_SUMMARY_FORM")) cut = e[0] == '0' ? 1 : e[0] == '1' ? 0x7fffffff : 64;
        DevBuf *sm = c.sm;
        const size_t np = (size_t)n_pairs;
        if ((rc = sm[SM_OUT].ensure(np * sizeof(gnx_aln_summary)))) return fail(rc);
        auto run = [&]() -> int {
            SumArgs a;
            int pk, r; // pk: which side the kernels read packed
            if ((r = sum_upload(c, st, prm, n_pairs, sa, sb, ops, ops_off, a, pk))) return r;
            a.gap_open = prm->gap_open; a.gap_extend = prm->gap_extend; a.cut = cut; a.affine = affine;
            int64_t *d_carry = (int64_t *)sm[SM_MISC].p + 1;
            auto launch = [&](bool write) -> int {
                for (int64_t b = 0; b < n_pairs; b += sub) {
                    const int64_t cnt = std::min(sub, n_pairs - b);
                    const SumArgs s = sum_sub_args(a, sm, b, cnt);
                    const dim3 grid((unsigned)std::min<int64_t>((cnt + 3) / 4, 1 << 20));
                    if (write) {
                        if (pk == 1) hipLaunchKernelGGL((aln_summary_kernel<true, 1>), grid, dim3(256), 0, st, s);
                        else if (pk == 2) hipLaunchKernelGGL((aln_summary_kernel<true, 2>), grid, dim3(256), 0, st, s);
                        else hipLaunchKernelGGL((aln_summary_kernel<true, 0>), grid, dim3(256), 0, st, s);
                    } else {
                        launch_sum_bases(s, pk, sa, sb, b, cnt, st);
                        if (pk == 1) hipLaunchKernelGGL((aln_summary_kernel<false, 1>), grid, dim3(256), 0, st, s);
                        else if (pk == 2) hipLaunchKernelGGL((aln_summary_kernel<false, 2>), grid, dim3(256), 0, st, s);
                        else hipLaunchKernelGGL((aln_summary_kernel<false, 0>), grid, dim3(256), 0, st, s);
                    }
                    HIPCHK(hipGetLastError());
                    int r;
                    if (!write && xc && (r = launch_scan(s.nx, (int)cnt, (int64_t *)sm[SM_XOFF].p + b, d_carry, st))) return r;
                    t.n_launches++;
                }
                return GNX_OK;
            };
            HIPCHK(hipEventRecord(c.ev[0], st));
            if ((r = launch(false))) return r;
            HIPCHK(hipEventRecord(c.ev[1], st));
            int ef = 0;
            HIPCHK(hipMemcpyAsync(&ef, sm[SM_MISC].p, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_out.data(), sm[SM_OUT].p, np * sizeof(gnx_aln_summary), hipMemcpyDeviceToHost, st));
            if (xc) HIPCHK(hipMemcpyAsync(xoff, sm[SM_XOFF].p, (np + 1) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st)); // (also: the sources are pageable memory of the caller -- no return while a copy may still read them)
            if (ef & 1) { set_err("a base >= 5 was found: the reference would panic (index out of range)%s", ""); return GNX_EBASE; }
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
            t.fill_ms = ms;
            if (xc) {
                n_x = xoff[n_pairs];
                xops = (gnx_cigar *)g_pool.get((size_t)std::max<int64_t>(n_x, 1) * sizeof(gnx_cigar));
                if (!xops) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
                if (n_x > 0) {
                    if ((r = sm[SM_XOPS].ensure((size_t)n_x * sizeof(gnx_cigar)))) return r;
                    a.xops = (gnx_cigar *)sm[SM_XOPS].p;
                    HIPCHK(hipEventRecord(c.ev[2], st));
                    if ((r = launch(true))) return r;
                    HIPCHK(hipEventRecord(c.ev[3], st));
                    HIPCHK(hipMemcpyAsync(xops, sm[SM_XOPS].p, (size_t)n_x * sizeof(gnx_cigar), hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                    HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
                    t.fill_ms += ms;
                }
            }
            return GNX_OK;
        };
        if ((rc = run())) { (void)hipStreamSynchronize(st); return fail(rc); }
    } else if (xc) {
        xops = (gnx_cigar *)g_pool.get(sizeof(gnx_cigar));
        if (!xops) { set_err("pinned host allocation failed%s", ""); return fail(GNX_ENOMEM); }
    }
    if (n_pairs > 0) memcpy(out, h_out.data(), (size_t)n_pairs * sizeof(gnx_aln_summary));
    if (xc) { *out_xops = xops; *out_xops_off = xoff; }
    t.dominant_ms = t.total_ms = t.fill_ms; t.dominant_launches = t.n_launches;
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

// ---- gnx_md_*: the MD strings of CIGARs walked against their sequences (aln_md.hip.h; contract: gnx_align.h) ----------------------
// gnx_summarize_*'s host flow with bytes where it has extended runs: the same checks, the same uploads into the same buffers (the
// bytes go where the extended runs go), the base check, aln_md_kernel<false> and the scan per sub-batch of GNX_HOST_SUB pairs
// (GNX_MD_SUB=<pairs> overrides the cut), one read-back of the flags and offsets that sizes the output, aln_md_kernel<true>.
int run_md(const gnx_params *prm, int64_t n_pairs, const SeqSide &sa, const SeqSide &sb, const gnx_cigar *ops, const int64_t *ops_off, char **out_md, int64_t **out_md_off) {
    const auto t_entry = std::chrono::steady_clock::now();
    int rc;
    int64_t cells = 0;
    if ((rc = check_cigar_call(prm, n_pairs, sa, sb, ops, ops_off, out_md && out_md_off, true, cells))) return rc;
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    if ((rc = check_resident_windows(c, n_pairs, sa, sb))) return rc;
    hipStream_t st = c.own_stream;
    char *md = nullptr;
    int64_t *off = (int64_t *)g_pool.get((size_t)(n_pairs + 1) * 8);
    if (!off) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
    off[0] = 0;
    auto fail = [&](int r) { g_pool.put(off); if (md) g_pool.put(md); return r; };
    gnx_timing t = {};
    t.fast_path = 13; t.cells = cells; t.n_contexts = 1;
    if (n_pairs > 0) {
        int64_t sub = gnx_host_sub(getenv("GNX_HOST_SUB"));
        if (const char *e = getenv("GNX_MD_SUB")) sub = std::max<int64_t>(atoll(e), 1);
        int cut = 64;
        if (const char *e = getenv("GNX_MD_FORM")) cut = e[0] == '0' ? 1 : e[0] == '1' ? 0x7fffffff : 64;
        DevBuf *sm = c.sm;
        const size_t np = (size_t)n_pairs;
        auto run = [&]() -> int {
            MdArgs a;
            a.md = nullptr;
            int pk, r;
            if ((r = sum_upload(c, st, prm, n_pairs, sa, sb, ops, ops_off, a.s, pk))) return r;
            a.s.cut = cut;
            int64_t *d_carry = (int64_t *)sm[SM_MISC].p + 1;
            auto launch = [&](bool write) -> int {
                for (int64_t b = 0; b < n_pairs; b += sub) {
                    const int64_t cnt = std::min(sub, n_pairs - b);
                    MdArgs s = a;
                    s.s = sum_sub_args(a.s, sm, b, cnt);
                    const dim3 grid((unsigned)std::min<int64_t>((cnt + 3) / 4, 1 << 20));
                    if (write) {
                        if (pk == 1) hipLaunchKernelGGL((aln_md_kernel<true, 1>), grid, dim3(256), 0, st, s);
                        else if (pk == 2) hipLaunchKernelGGL((aln_md_kernel<true, 2>), grid, dim3(256), 0, st, s);
                        else hipLaunchKernelGGL((aln_md_kernel<true, 0>), grid, dim3(256), 0, st, s);
                    } else {
                        launch_sum_bases(s.s, pk, sa, sb, b, cnt, st);
                        if (pk == 1) hipLaunchKernelGGL((aln_md_kernel<false, 1>), grid, dim3(256), 0, st, s);
                        else if (pk == 2) hipLaunchKernelGGL((aln_md_kernel<false, 2>), grid, dim3(256), 0, st, s);
                        else hipLaunchKernelGGL((aln_md_kernel<false, 0>), grid, dim3(256), 0, st, s);
                    }
                    HIPCHK(hipGetLastError());
                    if (!write && (r = launch_scan(s.s.nx, (int)cnt, (int64_t *)sm[SM_XOFF].p + b, d_carry, st))) return r;
                    t.n_launches++;
                }
                return GNX_OK;
            };
            HIPCHK(hipEventRecord(c.ev[0], st));
            if ((r = launch(false))) return r;
            HIPCHK(hipEventRecord(c.ev[1], st));
            int ef = 0;
            HIPCHK(hipMemcpyAsync(&ef, sm[SM_MISC].p, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(off, sm[SM_XOFF].p, (np + 1) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st)); // (also: the sources are pageable memory of the caller -- no return while a copy may still read them)
            if (ef & 1) { set_err("a base >= 5 was found: the reference would panic (index out of range)%s", ""); return GNX_EBASE; }
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
            t.fill_ms = ms;
            const int64_t n_md = off[n_pairs]; // (at least one byte per pair)
            md = (char *)g_pool.get((size_t)n_md);
            if (!md) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
            if ((r = sm[SM_XOPS].ensure((size_t)n_md + 64))) return r;
            a.md = (char *)sm[SM_XOPS].p;
            HIPCHK(hipEventRecord(c.ev[2], st));
            if ((r = launch(true))) return r;
            HIPCHK(hipEventRecord(c.ev[3], st));
            HIPCHK(hipMemcpyAsync(md, sm[SM_XOPS].p, (size_t)n_md, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
            t.fill_ms += ms;
            return GNX_OK;
        };
        if ((rc = run())) { (void)hipStreamSynchronize(st); return fail(rc); }
    } else {
        md = (char *)g_pool.get(1);
        if (!md) { set_err("pinned host allocation failed%s", ""); return fail(GNX_ENOMEM); }
    }
    *out_md = md; *out_md_off = off;
    t.dominant_ms = t.total_ms = t.fill_ms; t.dominant_launches = t.n_launches;
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

// ---- gnx_pileup_*: per-position counts of placed reads beside the resident reference, and the calls they give (pileup.hip.h; contract: gnx_align.h) ----
// One pile, on context 0, owned by the resident reference (drop_pile).  Every entry takes the context's lock before it looks at the
// pile; "no open pile" needs no device and is answered before ensure_init.
int need_pile(const Ctx &c) {
    if (c.pl_len >= 0) return GNX_OK;
    set_err("no open pile: call gnx_pileup_open first%s", "");
    return GNX_EINVAL;
}

int run_pile_open(int64_t region_start, int64_t region_len) {
    if (region_start < 0 || region_len < 1) { set_err("a pile's region holds at least one position of the reference%s", ""); return GNX_EINVAL; }
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = ensure_init())) return rc;
    if (c.ref_len < 0) { set_err("no resident reference: call gnx_set_reference first%s", ""); return GNX_EINVAL; }
    if (region_len > c.ref_len - region_start) { set_err("the region ends outside the reference of %s%lld bases", "", (long long)c.ref_len); return GNX_EINVAL; }
    // beside the open pile, which stays as it was when this one does not fit
    const size_t bytes = (size_t)region_len * PILE_PLANES * sizeof(int);
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); set_err("device allocation of %s%lld bytes failed", "", (long long)bytes); return GNX_ENOMEM; }
    if (hipMemsetAsync(q, 0, bytes, c.own_stream) != hipSuccess || hipStreamSynchronize(c.own_stream) != hipSuccess) {
        set_err_hip(hipGetLastError(), __FILE__, __LINE__);
        (void)hipFree(q);
        return GNX_EDEVICE;
    }
    c.pl_tab.release();
    drop_pile_log(c); // (a new pile does not track until it is told to)
    drop_pile_qual(c);
    c.pl_tab.p = q; c.pl_tab.cap = bytes;
    c.pl_start = region_start; c.pl_len = region_len; c.pl_reads = 0;
    return GNX_OK;
}

// The log of a tracking pile holds at least `events` events afterwards.  It grows by allocate-copy-free: the new planes are allocated
// beside the old ones, which are freed only when the copy has landed; a failure is GNX_ENOMEM with the log as it was.
int pile_log_reserve(Ctx &c, hipStream_t st, int64_t events) {
    if (events <= c.pl_log_cap) return GNX_OK;
    const int64_t cap = c.pl_log_cap == 0 ? events : events + events / 8 + 64; // (the first log is what the caller reserved)
    void *q = nullptr;
    if (hipMalloc(&q, (size_t)cap * 16) != hipSuccess) { (void)hipGetLastError(); set_err("device allocation of %s%lld bytes failed", "", (long long)cap * 16); return GNX_ENOMEM; }
    if (c.pl_events > 0) {
        const size_t used = (size_t)c.pl_events * 8;
        if (hipMemcpyAsync(q, c.pl_log.p, used, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync((unsigned long long *)q + cap, (const unsigned long long *)c.pl_log.p + c.pl_log_cap, used, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            set_err_hip(hipGetLastError(), __FILE__, __LINE__);
            (void)hipFree(q);
            return GNX_EDEVICE;
        }
    }
    c.pl_log.release();
    c.pl_log.p = q; c.pl_log.cap = (size_t)cap * 16;
    c.pl_log_cap = cap;
    return GNX_OK;
}

int run_pile_track(int64_t reserve_events) {
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c))) return rc;
    if (reserve_events < 0 || reserve_events > INT32_MAX) { set_err("reserve_events: 0 (a default) .. 2^31 - 1%s", ""); return GNX_EINVAL; }
    if (c.pl_reads != 0) { set_err("gnx_pileup_track_alleles: reads have been added to this pile (%s%lld): their alleles are gone", "", (long long)c.pl_reads); return GNX_EINVAL; }
    if ((rc = ensure_init())) return rc;
    hipStream_t st = c.own_stream;
    // the cursor first: a pile tracks only when both allocations stand (a second call on an empty pile keeps a log that is large enough)
    if (!c.pl_cur.p && hipMalloc(&c.pl_cur.p, 8) != hipSuccess) { (void)hipGetLastError(); c.pl_cur.p = nullptr; set_err("device allocation of %s%lld bytes failed", "", 8); return GNX_ENOMEM; }
    c.pl_cur.cap = 8;
    HIPCHK(hipMemsetAsync(c.pl_cur.p, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    c.pl_events = 0;
    if ((rc = pile_log_reserve(c, st, reserve_events > 0 ? reserve_events : (int64_t)1 << 16))) return rc;
    c.pl_track = true;
    return GNX_OK;
}

// gnx_pileup_track_qualities: four zeroed qsum planes beside the 14, allocated before anything changes (a second call on an empty pile
// keeps the planes, zeroes them again and takes the new min_baseq)
int run_pile_track_qual(int32_t min_baseq) {
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c))) return rc;
    if (min_baseq < 0 || min_baseq > QUAL_MAX) { set_err("min_baseq: 0 .. 93, not %s%lld", "", (long long)min_baseq); return GNX_EINVAL; }
    if (c.pl_reads != 0) { set_err("gnx_pileup_track_qualities: reads have been added to this pile (%s%lld): their qualities are gone", "", (long long)c.pl_reads); return GNX_EINVAL; }
    if ((rc = ensure_init())) return rc;
    const size_t bytes = (size_t)c.pl_len * QUAL_PLANES * sizeof(int);
    void *q = c.pl_qsum.p;
    if (!q && hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); set_err("device allocation of %s%lld bytes failed", "", (long long)bytes); return GNX_ENOMEM; }
    if (hipMemsetAsync(q, 0, bytes, c.own_stream) != hipSuccess || hipStreamSynchronize(c.own_stream) != hipSuccess) {
        set_err_hip(hipGetLastError(), __FILE__, __LINE__);
        if (!c.pl_qsum.p) (void)hipFree(q);
        return GNX_EDEVICE;
    }
    c.pl_qsum.p = q; c.pl_qsum.cap = bytes;
    c.pl_qual = true; c.pl_minq = min_baseq;
    return GNX_OK;
}

// gnx_md_batch_by_offset's checks and uploads (sa = the windows, sb = the reads), the base check over every launch cut, ONE read-back of
// its flag -- nothing may change the pile before every error is known --, then pile_add_kernel per sub-batch of GNX_HOST_SUB pairs
// (GNX_PILE_SUB=<pairs> overrides the cut).  On a tracking pile the log is grown first -- beside the old one, before the first launch that could
// change the pile -- and allele_log_kernel follows pile_add_kernel over the same buffers and the same cuts.
// with_qual: gnx_pileup_add_by_offset_qual -- the entry and the pile must agree; the qualities go up beside the reads and qual_add_kernel
// (pile_qual.hip.h) takes pile_add_kernel's place.  A plain pile runs nothing of that.
int run_pile_add(const gnx_params *prm, int64_t n_pairs, const SeqSide &sa, const SeqSide &sb, const uint8_t *strand, const gnx_cigar *ops, const int64_t *ops_off,
                 const uint8_t *use, const uint8_t *qual_cat, bool with_qual) {
    const auto t_entry = std::chrono::steady_clock::now();
    int rc;
    int64_t cells = 0;
    if ((rc = check_cigar_call(prm, n_pairs, sa, sb, ops, ops_off, strand != nullptr || n_pairs == 0, true, cells))) return rc;
    int64_t n_use = 0, gap_runs = 0, max_ins = 0, max_del = 0; // gap_runs: the I and D runs of non-zero length -- no call logs more events
    cells = 0; // of the added pairs
    for (int64_t q = 0; q < n_pairs; q++) {
        if (strand[q] > 1) { set_err("strand byte > 1 at pair %s%lld", "", (long long)q); return GNX_EINVAL; }
        if (use && !use[q]) continue;
        n_use++;
        int64_t ins = 0, del = 0;
        for (int64_t x = ops_off[q]; x < ops_off[q + 1]; x++) {
            cells += ops[x].run_length;
            if (ops[x].run_length > 0 && ops[x].op != GNX_COL_M) { gap_runs++; (ops[x].op == GNX_COL_I ? ins : del) += ops[x].run_length; }
        }
        max_ins = std::max(max_ins, ins); max_del = std::max(max_del, del);
    }
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    if ((rc = need_pile(c))) return rc;
    if (with_qual != c.pl_qual) {
        if (with_qual) set_err("gnx_pileup_add_by_offset_qual: the open pile does not track qualities: call gnx_pileup_track_qualities before the first add%s", "");
        else set_err("gnx_pileup_add_by_offset: the open pile tracks qualities: its reads come through gnx_pileup_add_by_offset_qual%s", "");
        return GNX_EINVAL;
    }
    if (c.pl_qual && n_use > QUAL_MAX_READS - c.pl_reads) { set_err("more than %s%lld reads in one quality pile (a read adds up to 93 to an int32 sum)", "", (long long)QUAL_MAX_READS); return GNX_EINVAL; }
    if (n_use > (int64_t)INT32_MAX - c.pl_reads) { set_err("more than 2^31 - 1 reads in one pile (its counters are int32)%s", ""); return GNX_EINVAL; }
    if (c.pl_track && gap_runs > (int64_t)INT32_MAX - c.pl_events) { set_err("more than 2^31 - 1 indel events in one pile%s", ""); return GNX_EINVAL; }
    if (n_pairs == 0) return GNX_OK;
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    if ((rc = check_resident_windows(c, n_pairs, sa, sb))) return rc;
    hipStream_t st = c.own_stream;
    gnx_timing t = {};
    t.fast_path = 14; t.cells = cells; t.n_contexts = 1;
    int64_t sub = gnx_host_sub(getenv("GNX_HOST_SUB"));
    if (const char *e = getenv("GNX_PILE_SUB")) sub = std::max<int64_t>(atoll(e), 1);
    int64_t events = c.pl_events; // the log's cursor after this call
    int cut = 64;
    if (const char *e = getenv("GNX_PILE_FORM")) cut = e[0] == '0' ? 1 : e[0] == '1' ? 0x7fffffff : 64;
    DevBuf *sm = c.sm;
    const size_t np = (size_t)n_pairs;
    auto run = [&]() -> int {
        SumArgs a;
        int pk, r;
        if ((r = sum_upload(c, st, prm, n_pairs, sa, sb, ops, ops_off, a, pk))) return r;
        if ((r = c.pl_in.ensure(2 * np))) return r;
        HIPCHK(hipMemcpyAsync(c.pl_in.p, strand, np, hipMemcpyHostToDevice, st));
        if (use) HIPCHK(hipMemcpyAsync((uint8_t *)c.pl_in.p + np, use, np, hipMemcpyHostToDevice, st));
        if (c.pl_qual) { // the qualities beside the reads: the same layout, the same starts
            if ((r = c.pl_qin.ensure((size_t)sb.buf_len + 16))) return r;
            if (sb.buf_len > 0) HIPCHK(hipMemcpyAsync(c.pl_qin.p, qual_cat, (size_t)sb.buf_len, hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipEventRecord(c.ev[0], st));
        for (int64_t b = 0; b < n_pairs; b += sub) launch_sum_bases(sum_sub_args(a, sm, b, std::min(sub, n_pairs - b)), pk, sa, sb, b, std::min(sub, n_pairs - b), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c.ev[1], st));
        int ef = 0;
        HIPCHK(hipMemcpyAsync(&ef, sm[SM_MISC].p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st)); // (also: the sources are pageable memory of the caller -- no return while a copy may still read them)
        if (ef & 1) { set_err("a base >= 5 was found: the reference would panic (index out of range)%s", ""); return GNX_EBASE; }
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        t.fill_ms = ms;
        if (n_use == 0) return GNX_OK;
        if (c.pl_track && (r = pile_log_reserve(c, st, c.pl_events + gap_runs))) return r;
        PileArgs pa;
        pa.reads = (const uint8_t *)sm[SM_B].p; pa.ops = (const gnx_cigar *)sm[SM_OPS].p; pa.cut = cut;
        pa.pile = (int *)c.pl_tab.p; pa.region_start = c.pl_start; pa.region_len = c.pl_len;
        HIPCHK(hipEventRecord(c.ev[2], st));
        for (int64_t b = 0; b < n_pairs; b += sub) {
            const int64_t cnt = std::min(sub, n_pairs - b);
            pa.read_start = (const int64_t *)sm[SM_BS].p + b; pa.ref_start = (const int64_t *)sm[SM_AS].p + b; pa.ops_off = (const int64_t *)sm[SM_OFF].p + b;
            pa.strand = (const uint8_t *)c.pl_in.p + b; pa.use = use ? (const uint8_t *)c.pl_in.p + np + b : nullptr;
            pa.n_pairs = cnt;
            if (c.pl_qual) {
                QualAddArgs qa;
                qa.p = pa; qa.quals = (const uint8_t *)c.pl_qin.p; qa.qsum = (int *)c.pl_qsum.p; qa.min_baseq = c.pl_minq;
                hipLaunchKernelGGL(qual_add_kernel, dim3((unsigned)std::min<int64_t>((cnt + 3) / 4, 1 << 20)), dim3(256), 0, st, qa);
            } else {
                hipLaunchKernelGGL(pile_add_kernel, dim3((unsigned)std::min<int64_t>((cnt + 3) / 4, 1 << 20)), dim3(256), 0, st, pa);
            }
            HIPCHK(hipGetLastError());
            t.n_launches++;
        }
        HIPCHK(hipEventRecord(c.ev[3], st));
        t.dominant_launches = t.n_launches;
        if (c.pl_track) {
            PileAlleleArgs aa;
            aa.reads = pa.reads; aa.ops = pa.ops; aa.region_start = c.pl_start; aa.region_len = c.pl_len;
            aa.w0 = (unsigned long long *)c.pl_log.p; aa.w1 = aa.w0 + c.pl_log_cap; aa.cursor = (unsigned long long *)c.pl_cur.p; aa.cap = (unsigned long long)c.pl_log_cap;
            for (int64_t b = 0; b < n_pairs; b += sub) {
                const int64_t cnt = std::min(sub, n_pairs - b);
                aa.read_start = (const int64_t *)sm[SM_BS].p + b; aa.ref_start = (const int64_t *)sm[SM_AS].p + b; aa.ops_off = (const int64_t *)sm[SM_OFF].p + b;
                aa.strand = (const uint8_t *)c.pl_in.p + b; aa.use = use ? (const uint8_t *)c.pl_in.p + np + b : nullptr;
                aa.n_pairs = cnt;
                hipLaunchKernelGGL(allele_log_kernel, dim3((unsigned)std::min<int64_t>((cnt + 3) / 4, 1 << 20)), dim3(256), 0, st, aa);
                HIPCHK(hipGetLastError());
                t.n_launches++;
            }
            HIPCHK(hipEventRecord(c.ev[4], st));
            HIPCHK(hipMemcpyAsync(&events, c.pl_cur.p, 8, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
        t.fill_ms += ms; t.dominant_ms = ms; // (dominant_ms: pile_add_kernel alone; on a quality pile: qual_add_kernel alone)
        if (c.pl_track) { HIPCHK(hipEventElapsedTime(&ms, c.ev[3], c.ev[4])); t.fill_ms += ms; }
        return GNX_OK;
    };
    if ((rc = run())) { (void)hipStreamSynchronize(st); return rc; }
    c.pl_reads += n_use;
    if (c.pl_track && n_use > 0) {
        c.pl_events = events;
        const int ins_bits = max_ins == 0 ? 0 : max_ins <= PILE_SEQ_MAX ? 3 * (int)max_ins : 63;
        int len_bits = 0;
        while (len_bits < 62 && ((int64_t)1 << len_bits) <= std::max(max_ins, max_del)) len_bits++;
        c.pl_key_bits = std::max(c.pl_key_bits, std::max(ins_bits, len_bits));
    }
    t.total_ms = t.fill_ms;
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

// rows for the caller: the planes come down a slab of rows at a time and are transposed here
int run_pile_get(int64_t first, int64_t count, gnx_pile *out) {
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c))) return rc;
    if (first < 0 || count < 0 || count > c.pl_len - first || (count > 0 && !out)) { set_err("rows outside the pile's region%s", ""); return GNX_EINVAL; }
    if (count == 0) return GNX_OK;
    if ((rc = ensure_init())) return rc;
    const int64_t slab = std::min<int64_t>(count, (int64_t)1 << 20);
    std::vector<int> h((size_t)slab * PILE_PLANES);
    for (int64_t b = 0; b < count; b += slab) {
        const int64_t n = std::min(slab, count - b);
        for (int pl = 0; pl < PILE_PLANES; pl++)
            HIPCHK(hipMemcpyAsync(h.data() + (size_t)pl * (size_t)slab, (const int *)c.pl_tab.p + (size_t)pl * (size_t)c.pl_len + (size_t)(first + b), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c.own_stream));
        HIPCHK(hipStreamSynchronize(c.own_stream));
        for (int64_t k = 0; k < n; k++) {
            gnx_pile &row = out[b + k];
            for (int s = 0; s < 2; s++) {
                for (int x = 0; x < 5; x++) row.base[s][x] = h[(size_t)(s * 5 + x) * (size_t)slab + (size_t)k];
                row.del[s] = h[(size_t)(PILE_DEL + s) * (size_t)slab + (size_t)k];
                row.ins[s] = h[(size_t)(PILE_INS + s) * (size_t)slab + (size_t)k];
                row._reserved[s] = 0;
            }
        }
    }
    return GNX_OK;
}

// the qsum rows of a quality pile: [count][4], A C G T
int run_pile_get_qual(int64_t first, int64_t count, int32_t *out) {
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c))) return rc;
    if (!c.pl_qual) { set_err("the open pile does not track qualities: call gnx_pileup_track_qualities before the first add%s", ""); return GNX_EINVAL; }
    if (first < 0 || count < 0 || count > c.pl_len - first || (count > 0 && !out)) { set_err("rows outside the pile's region%s", ""); return GNX_EINVAL; }
    if (count == 0) return GNX_OK;
    if ((rc = ensure_init())) return rc;
    const int64_t slab = std::min<int64_t>(count, (int64_t)1 << 20);
    std::vector<int> h((size_t)slab * QUAL_PLANES);
    for (int64_t b = 0; b < count; b += slab) {
        const int64_t n = std::min(slab, count - b);
        for (int pl = 0; pl < QUAL_PLANES; pl++)
            HIPCHK(hipMemcpyAsync(h.data() + (size_t)pl * (size_t)slab, (const int *)c.pl_qsum.p + (size_t)pl * (size_t)c.pl_len + (size_t)(first + b), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c.own_stream));
        HIPCHK(hipStreamSynchronize(c.own_stream));
        for (int64_t k = 0; k < n; k++)
            for (int x = 0; x < QUAL_PLANES; x++) out[(b + k) * QUAL_PLANES + x] = h[(size_t)x * (size_t)slab + (size_t)k];
    }
    return GNX_OK;
}

// the ranges of gnx_pile_call_opts, for both call entries
bool pile_call_opts_ok(const gnx_pile_call_opts *o) {
    if (o->min_depth >= 1 && o->min_alt >= 1 && o->frac_num >= 1 && o->frac_num <= o->frac_den && o->frac_den <= (1 << 20) && o->both_strands >= 0 && o->both_strands <= 1) return true;
    set_err("gnx_pile_call_opts: min_depth >= 1, min_alt >= 1, 1 <= frac_num <= frac_den <= 2^20, both_strands 0 or 1%s", "");
    return false;
}

// pile_call_kernel<false>, the scan of the tiles' counts, one read-back that sizes the list, pile_call_kernel<true>
int run_pile_calls(const gnx_pile_call_opts *o, gnx_pile_call **out_calls, int64_t *out_n) {
    const auto t_entry = std::chrono::steady_clock::now();
    if (!o || !out_calls || !out_n) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if (!pile_call_opts_ok(o)) return GNX_EINVAL;
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c))) return rc;
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    hipStream_t st = c.own_stream;
    gnx_timing t = {};
    t.fast_path = 15; t.cells = c.pl_len; t.n_contexts = 1;
    const int64_t n_tiles = (c.pl_len + PILE_TILE - 1) / PILE_TILE;
    gnx_pile_call *calls = nullptr;
    int64_t total = 0;
    auto run = [&]() -> int {
        int r;
        if ((r = c.pl_cnt.ensure((size_t)(n_tiles + 1) * 8)) || (r = c.pl_off.ensure((size_t)(n_tiles + 1) * 8))) return r;
        int64_t *d_carry = (int64_t *)c.pl_cnt.p + n_tiles;
        HIPCHK(hipMemsetAsync(d_carry, 0, 8, st));
        PileCallArgs a;
        memset(&a, 0, sizeof(a));
        a.kp.b2 = (const unsigned *)c.ref.p; a.kp.bflag = (const unsigned long long *)c.ref_flag.p; a.kp.brank = (const unsigned *)c.ref_rank.p; a.kp.bexc = (const unsigned long long *)c.ref_exc.p;
        a.pile = (const int *)c.pl_tab.p; a.region_start = c.pl_start; a.region_len = c.pl_len; a.n_tiles = n_tiles;
        a.min_depth = o->min_depth; a.min_alt = o->min_alt; a.frac_num = o->frac_num; a.frac_den = o->frac_den; a.both_strands = o->both_strands;
        a.cnt = (int64_t *)c.pl_cnt.p; a.off = (const int64_t *)c.pl_off.p;
        const dim3 grid((unsigned)std::min<int64_t>((n_tiles + 3) / 4, 1 << 20));
        HIPCHK(hipEventRecord(c.ev[0], st));
        hipLaunchKernelGGL(pile_call_kernel<false>, grid, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        if ((r = launch_scan(a.cnt, (int)n_tiles, (int64_t *)c.pl_off.p, d_carry, st))) return r;
        HIPCHK(hipEventRecord(c.ev[1], st));
        HIPCHK(hipMemcpyAsync(&total, (const int64_t *)c.pl_off.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        t.fill_ms = ms; t.n_launches = 1;
        calls = (gnx_pile_call *)g_pool.get((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_pile_call));
        if (!calls) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
        if (total > 0) {
            if ((r = c.pl_calls.ensure((size_t)total * sizeof(gnx_pile_call)))) return r;
            a.out = (gnx_pile_call *)c.pl_calls.p;
            HIPCHK(hipEventRecord(c.ev[2], st));
            hipLaunchKernelGGL(pile_call_kernel<true>, grid, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c.ev[3], st));
            HIPCHK(hipMemcpyAsync(calls, c.pl_calls.p, (size_t)total * sizeof(gnx_pile_call), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
            t.fill_ms += ms; t.n_launches = 2;
        }
        return GNX_OK;
    };
    if ((rc = run())) { (void)hipStreamSynchronize(st); if (calls) g_pool.put(calls); return rc; }
    *out_calls = calls; *out_n = total;
    t.dominant_ms = t.total_ms = t.fill_ms; t.dominant_launches = t.n_launches;
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

// gnx_pileup_genotypes: run_pile_calls' pattern around geno_call_kernel -- the count pass, the scan of the tiles' counts, one read-back
// that sizes the list, the write pass
int run_pile_genotypes(const gnx_geno_opts *o, gnx_pile_genotype **out_recs, int64_t *out_n) {
    const auto t_entry = std::chrono::steady_clock::now();
    if (!o || !out_recs || !out_n) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if (o->min_depth < 1 || o->min_qual < 0 || o->prior_het < 0 || o->prior_het > (1 << 20) || o->prior_hom < 0 || o->prior_hom > (1 << 20)) {
        set_err("gnx_geno_opts: min_depth >= 1, min_qual >= 0, 0 <= prior_het, prior_hom <= 2^20%s", "");
        return GNX_EINVAL;
    }
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c))) return rc;
    if (!c.pl_qual) { set_err("the open pile does not track qualities: call gnx_pileup_track_qualities before the first add%s", ""); return GNX_EINVAL; }
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    hipStream_t st = c.own_stream;
    gnx_timing t = {};
    t.fast_path = 20; t.cells = c.pl_len; t.n_contexts = 1;
    const int64_t n_tiles = (c.pl_len + PILE_TILE - 1) / PILE_TILE;
    gnx_pile_genotype *recs = nullptr;
    int64_t total = 0;
    auto run = [&]() -> int {
        int r;
        if ((r = c.pl_cnt.ensure((size_t)(n_tiles + 1) * 8)) || (r = c.pl_off.ensure((size_t)(n_tiles + 1) * 8))) return r;
        int64_t *d_carry = (int64_t *)c.pl_cnt.p + n_tiles;
        HIPCHK(hipMemsetAsync(d_carry, 0, 8, st));
        GenoCallArgs a;
        memset(&a, 0, sizeof(a));
        a.kp.b2 = (const unsigned *)c.ref.p; a.kp.bflag = (const unsigned long long *)c.ref_flag.p; a.kp.brank = (const unsigned *)c.ref_rank.p; a.kp.bexc = (const unsigned long long *)c.ref_exc.p;
        a.pile = (const int *)c.pl_tab.p; a.qsum = (const int *)c.pl_qsum.p; a.region_start = c.pl_start; a.region_len = c.pl_len; a.n_tiles = n_tiles;
        a.o.min_depth = o->min_depth; a.o.min_qual = o->min_qual; a.o.prior_het = o->prior_het; a.o.prior_hom = o->prior_hom;
        a.cnt = (int64_t *)c.pl_cnt.p; a.off = (const int64_t *)c.pl_off.p;
        const dim3 grid((unsigned)std::min<int64_t>((n_tiles + 3) / 4, 1 << 20));
        HIPCHK(hipEventRecord(c.ev[0], st));
        hipLaunchKernelGGL(geno_call_kernel<false>, grid, dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        if ((r = launch_scan(a.cnt, (int)n_tiles, (int64_t *)c.pl_off.p, d_carry, st))) return r;
        HIPCHK(hipEventRecord(c.ev[1], st));
        HIPCHK(hipMemcpyAsync(&total, (const int64_t *)c.pl_off.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
        t.fill_ms = ms; t.n_launches = 1;
        recs = (gnx_pile_genotype *)g_pool.get((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_pile_genotype));
        if (!recs) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
        if (total > 0) {
            if ((r = c.pl_geno.ensure((size_t)total * sizeof(gnx_pile_genotype)))) return r;
            a.out = (gnx_pile_genotype *)c.pl_geno.p;
            HIPCHK(hipEventRecord(c.ev[2], st));
            hipLaunchKernelGGL(geno_call_kernel<true>, grid, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c.ev[3], st));
            HIPCHK(hipMemcpyAsync(recs, c.pl_geno.p, (size_t)total * sizeof(gnx_pile_genotype), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
            t.fill_ms += ms; t.n_launches = 2;
        }
        return GNX_OK;
    };
    if ((rc = run())) { (void)hipStreamSynchronize(st); if (recs) g_pool.put(recs); return rc; }
    *out_recs = recs; *out_n = total;
    t.dominant_ms = t.total_ms = t.fill_ms; t.dominant_launches = t.n_launches;
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

int need_tracking(const Ctx &c) {
    if (c.pl_track) return GNX_OK;
    set_err("the open pile does not track alleles: call gnx_pileup_track_alleles before the first add%s", "");
    return GNX_EINVAL;
}

// The distinct alleles of the log, ordered and counted, left in c.pl_al on the device: two stable radix sorts of the log's planes into
// scratch (by w1, then by w0: the order is (pos, kind, key, strand)), allele_reduce_kernel<false>, the scan of the tiles' counts,
// one read-back that sizes the array, allele_reduce_kernel<true>.  The log is only read.
// norm (the ..._norm entries): norm_shift_kernel first writes every event, left-normalised, into the two planes of
// c.pl_norm, and the sorts read those.  Their bit ranges hold: a rotated sequence has its digits, a position only shrinks.  norm_ms is
// that kernel alone.  GNX_NORM_COOP=0: every lane finishes its event alone (tests; the results do not depend on it).
int pile_alleles_device(Ctx &c, hipStream_t st, int64_t &n_alleles, gnx_timing &t, bool norm = false, float *norm_ms = nullptr) {
    const int64_t n = c.pl_events;
    n_alleles = 0;
    if (n == 0) return GNX_OK;
    int r;
    for (int k = 0; k < 4; k++) if ((r = c.pl_sort[k].ensure((size_t)n * 8))) return r;
    unsigned long long *w0 = (unsigned long long *)c.pl_log.p, *w1 = w0 + c.pl_log_cap;
    if (norm) {
        if ((r = c.pl_norm.ensure((size_t)n * 16))) return r;
        NormArgs na;
        memset(&na, 0, sizeof(na));
        na.kp.b2 = (const unsigned *)c.ref.p; na.kp.bflag = (const unsigned long long *)c.ref_flag.p; na.kp.brank = (const unsigned *)c.ref_rank.p; na.kp.bexc = (const unsigned long long *)c.ref_exc.p;
        na.w0 = w0; na.w1 = w1; na.o0 = (unsigned long long *)c.pl_norm.p; na.o1 = na.o0 + n;
        na.n = n; na.region_start = c.pl_start; na.ref_len = c.ref_len;
        const char *e = getenv("GNX_NORM_COOP");
        na.coop = e && e[0] == '0' ? 0 : 1;
        HIPCHK(hipEventRecord(c.ev[4], st));
        hipLaunchKernelGGL(norm_shift_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 20)), dim3(256), 0, st, na);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c.ev[5], st));
        t.n_launches++;
        w0 = na.o0; w1 = na.o1;
    }
    unsigned long long *s_w1 = (unsigned long long *)c.pl_sort[0].p, *s_w0 = (unsigned long long *)c.pl_sort[1].p;   // ordered by w1
    unsigned long long *o_w0 = (unsigned long long *)c.pl_sort[2].p, *o_w1 = (unsigned long long *)c.pl_sort[3].p;   // ordered by (w0, w1)
    // the bits that can differ: the strand and the longest key of any added pair; the region's positions and the kind
    const unsigned bits1 = (unsigned)std::min(64, c.pl_key_bits + 1);
    unsigned bits0 = 2;
    while (bits0 < 64 && ((uint64_t)1 << (bits0 - 2)) < (uint64_t)c.pl_len) bits0++;
    size_t tmp1 = 0, tmp0 = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp1, w1, s_w1, w0, s_w0, (size_t)n, 0u, bits1, st));
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp0, s_w0, o_w0, s_w1, o_w1, (size_t)n, 0u, bits0, st));
    size_t tmp_bytes = std::max(tmp1, tmp0);
    if ((r = c.pl_sort[4].ensure(std::max<size_t>(tmp_bytes, 8)))) return r;
    const int64_t n_tiles = (n + PILE_TILE - 1) / PILE_TILE;
    if ((r = c.pl_cnt.ensure((size_t)(n_tiles + 1) * 8)) || (r = c.pl_off.ensure((size_t)(n_tiles + 1) * 8))) return r;
    int64_t *d_carry = (int64_t *)c.pl_cnt.p + n_tiles;
    HIPCHK(hipMemsetAsync(d_carry, 0, 8, st));
    HIPCHK(hipEventRecord(c.ev[0], st));
    HIPCHK(rocprim::radix_sort_pairs(c.pl_sort[4].p, tmp_bytes, w1, s_w1, w0, s_w0, (size_t)n, 0u, bits1, st)); // stable LSD radix sorts: the second keeps the first's order within a w0
    HIPCHK(rocprim::radix_sort_pairs(c.pl_sort[4].p, tmp_bytes, s_w0, o_w0, s_w1, o_w1, (size_t)n, 0u, bits0, st));
    PileReduceArgs a;
    a.w0 = o_w0; a.w1 = o_w1; a.n = n; a.n_tiles = n_tiles; a.region_start = c.pl_start;
    a.cnt = (int64_t *)c.pl_cnt.p; a.off = (const int64_t *)c.pl_off.p; a.out = nullptr;
    const dim3 grid((unsigned)std::min<int64_t>((n_tiles + 3) / 4, 1 << 20));
    hipLaunchKernelGGL(allele_reduce_kernel<false>, grid, dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    if ((r = launch_scan(a.cnt, (int)n_tiles, (int64_t *)c.pl_off.p, d_carry, st))) return r;
    HIPCHK(hipEventRecord(c.ev[1], st));
    HIPCHK(hipMemcpyAsync(&n_alleles, (const int64_t *)c.pl_off.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    t.fill_ms += ms; t.n_launches += 3;
    if (norm) {
        HIPCHK(hipEventElapsedTime(&ms, c.ev[4], c.ev[5]));
        t.fill_ms += ms;
        if (norm_ms) *norm_ms = ms;
    }
    if ((r = c.pl_al.ensure((size_t)n_alleles * sizeof(gnx_pile_allele)))) return r;
    a.out = (gnx_pile_allele *)c.pl_al.p;
    HIPCHK(hipEventRecord(c.ev[2], st));
    hipLaunchKernelGGL(allele_reduce_kernel<true>, grid, dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c.ev[3], st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
    t.fill_ms += ms; t.n_launches++;
    return GNX_OK;
}

int run_pile_alleles(gnx_pile_allele **out, int64_t *out_n, bool norm) {
    const auto t_entry = std::chrono::steady_clock::now();
    if (!out || !out_n) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c)) || (rc = need_tracking(c))) return rc;
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    hipStream_t st = c.own_stream;
    gnx_timing t = {};
    t.fast_path = norm ? 18 : 16; t.cells = c.pl_events; t.n_contexts = 1;
    gnx_pile_allele *res = nullptr;
    int64_t total = 0;
    float norm_ms = 0;
    auto run = [&]() -> int {
        int r;
        if ((r = pile_alleles_device(c, st, total, t, norm, &norm_ms))) return r;
        res = (gnx_pile_allele *)g_pool.get((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_pile_allele));
        if (!res) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
        if (total > 0) {
            HIPCHK(hipMemcpyAsync(res, c.pl_al.p, (size_t)total * sizeof(gnx_pile_allele), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return GNX_OK;
    };
    if ((rc = run())) { (void)hipStreamSynchronize(st); if (res) g_pool.put(res); return rc; }
    *out = res; *out_n = total;
    t.dominant_ms = t.total_ms = t.fill_ms; t.dominant_launches = t.n_launches;
    if (norm) { t.dominant_ms = norm_ms; t.dominant_launches = c.pl_events > 0 ? 1 : 0; } // (dominant_ms: norm_shift_kernel alone)
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

// the alleles as above, then allele_call_kernel<false>, the scan, one read-back, allele_call_kernel<true> over the array the reduce left
int run_pile_indel_calls(const gnx_pile_call_opts *o, gnx_pile_indel_call **out_calls, int64_t *out_n, bool norm) {
    const auto t_entry = std::chrono::steady_clock::now();
    if (!o || !out_calls || !out_n) { set_err("bad argument%s", ""); return GNX_EINVAL; }
    if (!pile_call_opts_ok(o)) return GNX_EINVAL;
    Ctx &c = ctx_at(0);
    CtxScope scope(c);
    int rc;
    if ((rc = need_pile(c)) || (rc = need_tracking(c))) return rc;
    if ((rc = ensure_init())) return rc;
    g_transport = 0; g_bcast_ms = 0;
    hipStream_t st = c.own_stream;
    gnx_timing t = {}, ta = {};
    t.fast_path = norm ? 19 : 17; t.n_contexts = 1;
    gnx_pile_indel_call *calls = nullptr;
    int64_t total = 0;
    float norm_ms = 0;
    auto run = [&]() -> int {
        int r;
        int64_t n = 0;
        if ((r = pile_alleles_device(c, st, n, ta, norm, &norm_ms))) return r;
        t.cells = n;
        calls = nullptr;
        if (n > 0) {
            const int64_t n_tiles = (n + PILE_TILE - 1) / PILE_TILE;
            if ((r = c.pl_cnt.ensure((size_t)(n_tiles + 1) * 8)) || (r = c.pl_off.ensure((size_t)(n_tiles + 1) * 8))) return r;
            int64_t *d_carry = (int64_t *)c.pl_cnt.p + n_tiles;
            HIPCHK(hipMemsetAsync(d_carry, 0, 8, st));
            PileIndelCallArgs a;
            memset(&a, 0, sizeof(a));
            a.c.kp.b2 = (const unsigned *)c.ref.p; a.c.kp.bflag = (const unsigned long long *)c.ref_flag.p; a.c.kp.brank = (const unsigned *)c.ref_rank.p; a.c.kp.bexc = (const unsigned long long *)c.ref_exc.p;
            a.c.pile = (const int *)c.pl_tab.p; a.c.region_start = c.pl_start; a.c.region_len = c.pl_len; a.c.n_tiles = n_tiles;
            a.c.min_depth = o->min_depth; a.c.min_alt = o->min_alt; a.c.frac_num = o->frac_num; a.c.frac_den = o->frac_den; a.c.both_strands = o->both_strands;
            a.c.cnt = (int64_t *)c.pl_cnt.p; a.c.off = (const int64_t *)c.pl_off.p;
            a.alleles = (const gnx_pile_allele *)c.pl_al.p; a.n = n;
            const dim3 grid((unsigned)std::min<int64_t>((n_tiles + 3) / 4, 1 << 20));
            HIPCHK(hipEventRecord(c.ev[0], st));
            hipLaunchKernelGGL(allele_call_kernel<false>, grid, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
            if ((r = launch_scan(a.c.cnt, (int)n_tiles, (int64_t *)c.pl_off.p, d_carry, st))) return r;
            HIPCHK(hipEventRecord(c.ev[1], st));
            HIPCHK(hipMemcpyAsync(&total, (const int64_t *)c.pl_off.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
            t.fill_ms += ms; t.n_launches++;
            if (total > 0) {
                if ((r = c.pl_icalls.ensure((size_t)total * sizeof(gnx_pile_indel_call)))) return r;
                a.out = (gnx_pile_indel_call *)c.pl_icalls.p;
                HIPCHK(hipEventRecord(c.ev[2], st));
                hipLaunchKernelGGL(allele_call_kernel<true>, grid, dim3(256), 0, st, a);
                HIPCHK(hipGetLastError());
                HIPCHK(hipEventRecord(c.ev[3], st));
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(hipEventElapsedTime(&ms, c.ev[2], c.ev[3]));
                t.fill_ms += ms; t.n_launches++;
            }
        }
        calls = (gnx_pile_indel_call *)g_pool.get((size_t)std::max<int64_t>(total, 1) * sizeof(gnx_pile_indel_call));
        if (!calls) { set_err("pinned host allocation failed%s", ""); return GNX_ENOMEM; }
        if (total > 0) {
            HIPCHK(hipMemcpyAsync(calls, c.pl_icalls.p, (size_t)total * sizeof(gnx_pile_indel_call), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        return GNX_OK;
    };
    if ((rc = run())) { (void)hipStreamSynchronize(st); if (calls) g_pool.put(calls); return rc; }
    *out_calls = calls; *out_n = total;
    t.dominant_ms = t.fill_ms; t.dominant_launches = t.n_launches; // (dominant_ms: the call kernels alone; fill_ms: with the alleles' sort and reduce)
    if (norm) { t.dominant_ms = norm_ms; t.dominant_launches = c.pl_events > 0 ? 1 : 0; } // (the normalised query: norm_shift_kernel alone)
    t.fill_ms += ta.fill_ms; t.n_launches += ta.n_launches;
    t.total_ms = t.fill_ms;
    t.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_entry).count();
    c.timing = t;
    return GNX_OK;
}

// gnx_mapq_batch's rule for one read (gnx_align.h): the share of the score that the best other candidate does not reach, on a scale of 60
uint8_t mapq_of(int64_t score, int64_t second) {
    if (score <= 0) return 0;
    const int64_t s2 = second < 0 ? 0 : second; // (INT64_MIN, "no other candidate", is negative too)
    if (s2 >= score) return 0;
    const unsigned __int128 q = (unsigned __int128)60 * (uint64_t)(score - s2) / (uint64_t)score; // (60 * 2^63 does not fit 64 bits)
    return (uint8_t)std::min<uint64_t>(60, (uint64_t)q);
}

} // namespace
