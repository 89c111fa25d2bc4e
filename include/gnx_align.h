/*
 * gnx_align.h -- C ABI of libgonomics_align_hip.so: the MI355X (gfx950) drop-in for the pairwise DP hot
 * path of gonomics' `align` package.
 *
 * The reference (vertgenlab/gonomics) is pure Go and has no FFI layer.  The boundary it offers for this
 * path is the exported Go API of package align; each entry point below names the Go function(s) a cgo
 * shim would route through it (see INTEGRATION.md for the shim):
 *
 *   align.AffineGap(alpha, beta []dna.Base, scores [][]int64, gapOpen, gapExtend int64) (int64, []Cigar)
 *                                                              /root/reference/align/affineGap.go:59
 *   align.AffineGap_customizeCheckersize(..., checkersize_i, checkersize_j int)        affineGap.go:73
 *   align.ConstGap(alpha, beta, scores, gapPen) (int64, []Cigar)                        constGap.go:13
 *   align.ConstGap_customizeCheckersize(..., checkersize_i, checkersize_j int)         constGap.go:73
 *   align.AffineGap_highMem / align.AffineGapLocal(target, query, ...)      affineGap_highMem.go:99,105
 *   align.ConstGap_highMem                                                      constGap_highMem.go:11
 *   align.GoAffineGapLocalEngine (batched, FIFO)                              affineGap_highMem.go:120
 *
 * Conventions
 *   - bases are dna.Base bytes (A=0 C=1 G=2 T=3 N=4; /root/reference/dna/dna.go:5-21); any byte >= 5
 *     makes the Go code panic (index out of range on the 5x5 matrix) -> here: GNX_EBASE.
 *   - `scores` is the [][]int64 matrix flattened row-major: scores[alphaBase*5 + betaBase].
 *   - results are bit-exact with the reference: score (int64) and the run-length CIGAR in alignment
 *     order, including the low-memory checkerboard traceback quirks for n or m > checkersize.
 *   - gnx_cigar has the memory layout of Go's align.Cigar{RunLength int64; Op ColType(uint8)} on amd64.
 *   - inputs are borrowed and never written; outputs returned through gnx_cigar** / int64_t** are
 *     malloc'd by the library and released with gnx_free().
 *   - all functions return GNX_OK (0) or a GNX_E* code; gnx_last_error() gives the text.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry returns GNX_EDEVICE.
 */
#ifndef GNX_ALIGN_H
#define GNX_ALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNX_OK 0
#define GNX_EINVAL 1    /* bad argument (null pointer, negative size, unknown mode) */
#define GNX_EBASE 2     /* a base >= 5: the Go code would panic */
#define GNX_EEMPTY 3    /* empty sequence in a low-memory mode: the Go code would never terminate */
#define GNX_ERANGE 4    /* lengths x penalties exceed the int32 range of a mode that keeps absolute keys (the chunk / graph-extension variants).  The align functions
                         * proper (AffineGap*, ConstGap*, AffineGapLocal) have no range limit: what bounds them is (a) 2^30 - 1 bases per sequence -- longer: GNX_EINVAL --
                         * and (b) device memory: a pair whose bottom rows + snapshots fit neither the snapshot path nor row panels, or whose stored matrix (the int64
                         * kernel: AffineGapLocal, gapOpen > 0 beyond int32) does not fit, returns GNX_ENOMEM, not GNX_ERANGE.  A single oversize pair is given what the
                         * device has free, beyond the workspace limit of gnx_init (it cannot run any other way). */
#define GNX_EDEVICE 5   /* no HIP device / HIP runtime error */
#define GNX_ENOMEM 6    /* host or device allocation failed / workspace too small for one pair */
#define GNX_ECAPACITY 7 /* caller-provided device CIGAR buffer too small (device entry point) */
#define GNX_ETRACE 8    /* impossible traceback value: the Go code would log.Fatalf */
#define GNX_EDIVZERO 9  /* scoreColumnMatch over a column pair of gaps only: the Go code panics (integer divide by zero, multiAlign.go:101) */
#define GNX_ESTALE 10   /* gnx_seed_find_batch_gen: the resident seed index is not the generation named (set it again) */

/* align.ColType, /root/reference/align/align.go:12-18 */
#define GNX_COL_M 0
#define GNX_COL_I 1
#define GNX_COL_D 2

/* align.Cigar, /root/reference/align/align.go:21-24 */
typedef struct gnx_cigar {
    int64_t run_length;
    uint8_t op;
    uint8_t _pad[7];
} gnx_cigar;

typedef enum gnx_mode {
    GNX_AFFINE_GAP = 0,         /* AffineGap / AffineGap_customizeCheckersize (low-memory checkerboard semantics) */
    GNX_CONST_GAP = 1,          /* ConstGap / ConstGap_customizeCheckersize */
    GNX_AFFINE_GAP_HIGHMEM = 2, /* AffineGap_highMem */
    GNX_AFFINE_GAP_LOCAL = 3,   /* AffineGapLocal(target=alpha, query=beta), GoAffineGapLocalEngine */
    GNX_CONST_GAP_HIGHMEM = 4   /* ConstGap_highMem */
} gnx_mode;

typedef struct gnx_params {
    int32_t mode;          /* gnx_mode */
    int32_t _reserved;
    int64_t scores[25];    /* scores[a*5+b] */
    int64_t gap_open;      /* affine: gapOpen; const: gapPen */
    int64_t gap_extend;    /* affine: gapExtend; const: ignored */
    int64_t checkersize_i; /* low-memory modes only; 10000 for AffineGap / ConstGap */
    int64_t checkersize_j;
} gnx_params;

/* Per-call kernel timings of the most recent compute call of the process (context 0; with several contexts: the slowest
 * context's times, cells and bytes summed) -- HIP events on the stream the kernels ran on.  cells = sum over pairs of n*m. */
typedef struct gnx_timing {
    double fill_ms;      /* DP fill kernel(s): the dominant kernel */
    double traceback_ms; /* traceback count + scan + write kernels */
    double total_ms;     /* first launch to last kernel end */
    int64_t cells;
    int64_t n_launches;  /* number of fill launches (sub-batches) */
    int64_t trace_bytes; /* direction-matrix / checkpoint bytes written by the fill kernels */
    double dominant_ms;  /* summed duration of the dominant kernel's launches (fast path: the forward sweep; general
                            path: the fill kernel) -- what roofline.achieved is computed from */
    int64_t dominant_launches;
    int32_t fast_path;   /* 1: the affine fast path ran (short alpha x long beta; AffineGapLocal: short query x long target);
                            2: the constant-gap path without a stored direction matrix (const_long.hip.h); 0: full direction matrix;
                            3 / 4: the latency geometry (few pairs) in its int32 / int64 form; 5: the 64-lane affine snapshot path;
                            6: the constant-gap snapshot path in its 64-lane form; 7: the score-only sweep ran (gnx_score_* entries,
                            score_sweep.hip.h); 8: its AffineGapLocal variant ran (gnx_score_* with GNX_AFFINE_GAP_LOCAL, gnx_locate_*);
                            9: the score-only sweep with explicit cell scores ran (gnx_affine_gap_chunk_score_batch,
                            gnx_multiple_affine_gap_score_batch; n1_sweep.hip.h);
                            10: the local sweep (8) followed by the origin-carrying window DP ran (gnx_locate_span_*, gnx_best_pair_*;
                            span_origin.hip.h): fill_ms and total_ms cover both stages, dominant_ms is the sweep's.
                            11: gnx_seed_candidates ran (ref_seeds.hip.h): fill_ms = lookup + vote kernels, dominant_ms = the vote kernels, cells = seed
                            hits that voted, n_launches = vote sub-batches.
                            12: gnx_summarize_* ran (aln_summary.hip.h): fill_ms = dominant_ms = the summary kernels, cells = columns walked.
                            13: gnx_md_* ran (aln_md.hip.h): fill_ms = dominant_ms = the count and the write kernels, cells = columns walked.
                            Multi-context score calls report the maximum over contexts. */
    int32_t _pad;
    /* host-buffer entry points only (wall clock inside the library): */
    double host_ms;      /* entry to return of the whole call */
    double stage0_ms;    /* exposed upload of the first sub-batch (later ones run under the kernels) */
    double fetch_ms;     /* gather on device 0 + D2H of scores / offsets / CIGAR runs */
    /* multi-context calls (gnx_init_devices): */
    int32_t transport;   /* what carried the last broadcast / gather: 0 one context, 1 RCCL over xGMI, 2 peer copies (GNX_RCCL=0, or a
                            device listed twice), 3 peer copies AFTER a RCCL call failed (the text is in gnx_last_error) */
    int32_t n_contexts;  /* contexts the call was sharded over */
    double gather_ms;    /* the gather on device 0 alone (part of fetch_ms) */
    double bcast_ms;     /* broadcast of the shared beta buffer of this call (0 with a resident reference) */
} gnx_timing;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
int gnx_device_count(void);
/* Bind this process to HIP device `device` (one process per GPU).  workspace_bytes = upper bound for the
 * library's device scratch (direction matrices etc.); 0 picks a default from free memory. */
int gnx_init(int device, int64_t workspace_bytes);
/* One context per GPU inside ONE host process (what a Go program that calls align.* needs in order to use a whole node:
 * the reference's own parallel drivers are worker pools inside one process, /root/reference/genomeGraph/routines.go:12-65).
 * devices = NULL: devices 0 .. n_devices-1; n_devices <= 0: every visible GPU.  Afterwards the host-buffer entry points below cut
 * each batch into contiguous blocks of equal DP cells, one block per context (one worker thread each), upload a shared beta
 * buffer / the resident reference once and broadcast it with RCCL over xGMI, and gather scores / offsets / CIGARs on device 0
 * (grouped ncclSend / ncclRecv) in input order.  RCCL (librccl.so) is loaded with dlopen here, never for one GPU.
 * A device may be listed more than once (flow tests on a 1-GPU box): such contexts exchange by plain copies instead of RCCL.
 * Environment: GNX_RCCL=0 peer copies instead of RCCL; GNX_RCCL=1 build the communicator even for a single device. */
int gnx_init_devices(int n_devices, const int *devices, int64_t workspace_bytes_per_device);
int gnx_n_devices(void);
void gnx_shutdown(void);
/* Text of the calling thread's last error; if that thread has none, the most recent error of the process (cgo may run the failing
 * call and this one on different OS threads unless the shim pins the goroutine). */
const char *gnx_last_error(void);
void gnx_free(void *p);

/* ---- resident reference (configs C3 / C4: reads against windows of one genome) ------------------ */
/* Upload `ref` (dna.Base bytes) once; it stays on the device(s) until the next call or gnx_shutdown -- PACKED: 2 bits per base plus a
 * sparse list of the 64-base blocks that hold anything but A C G T (N; bytes >= 5, which make GNX_EBASE only when an alignment's
 * window touches them, like the Go code's panic): 4.4e9 bases take 1.1 GB of HBM and of RCCL broadcast instead of 4.4 GB.  It is
 * packed on device 0 (256 MB of bases at a time) and, with several contexts, broadcast over RCCL; the sweep kernels read the packed
 * words directly (len = 0 releases it).  Replaces passing the same target slice to every align.* call of a loop
 * (/root/reference/cmd/globalAlignmentAnchor/globalAlignmentAnchor.go:352-384 re-reads its two genomes per anchor). */
int gnx_set_reference(const uint8_t *ref, int64_t len);
/* What is resident: bases, bytes of device memory per context, 64-base blocks on the exception list. */
int gnx_reference_info(int64_t *out_bases, int64_t *out_device_bytes, int64_t *out_exception_blocks);
/* Synthetic reference of SURVEY 8d (config C3), generated on the device: base(pos) = 2 bits of splitmix64(seed ^ (pos / 32)) at
 * bit 2*(pos % 32), with an N run of 1000 bases at every multiple of 5e7 except 0.  For benchmarks and tests (3e9 bases do not
 * have to cross PCIe); nothing in the reference corresponds to it. */
int gnx_set_reference_synthetic(int64_t len, uint64_t seed);
/* Batch of reads (alpha_cat / alpha_off as in gnx_align_batch) against windows (ref_start[p], ref_len[p]) of the resident
 * reference: beta = reference[ref_start[p] .. ref_start[p] + ref_len[p]).  Only the reads and 16 bytes of window table per pair
 * cross PCIe.  Large batches are cut into sub-batches whose uploads run under the kernels of the sub-batch before (pinned
 * staging, second stream); results accumulate on the device and come back in one transfer into pinned memory (gnx_free). */
int gnx_align_batch_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *alpha_cat, const int64_t *alpha_off,
                              const int64_t *ref_start, const int64_t *ref_len,
                              int64_t *out_score, gnx_cigar **out_ops, int64_t **out_ops_off);

/* ---- host-buffer entry points (what the cgo shim binds) ------------------------------------------ */
/* Batch of independent pairs.  Pair p is alpha_cat[alpha_off[p] .. alpha_off[p+1]) vs
 * beta_cat[beta_off[p] .. beta_off[p+1]).  Outputs: out_score[n_pairs]; *out_ops = concatenated CIGARs,
 * (*out_ops_off)[n_pairs+1] their boundaries.  Replaces a serial loop of align.AffineGap* / ConstGap*
 * calls (cmd/globalAlignmentAnchor/globalAlignmentAnchor.go:352-384) and the FIFO engine
 * (affineGap_highMem.go:120-179): results are in input order. */
int gnx_align_batch(const gnx_params *p, int64_t n_pairs,
                    const uint8_t *alpha_cat, const int64_t *alpha_off,
                    const uint8_t *beta_cat, const int64_t *beta_off,
                    int64_t *out_score, gnx_cigar **out_ops, int64_t **out_ops_off);

/* Same, but each sequence is a window (start,len) into a shared buffer, so many pairs may reference one
 * resident chunk / genome (faChunkAlign-style read-vs-chunk batches). */
int gnx_align_batch_windows(const gnx_params *p, int64_t n_pairs,
                            const uint8_t *alpha_buf, int64_t alpha_buf_len, const int64_t *alpha_start, const int64_t *alpha_len,
                            const uint8_t *beta_buf, int64_t beta_buf_len, const int64_t *beta_start, const int64_t *beta_len,
                            int64_t *out_score, gnx_cigar **out_ops, int64_t **out_ops_off);

/* One pair == batch of 1: the body of the Go-signature functions.  Safe and EFFICIENT from many threads at once (a pool of
 * goroutines calling align.* is the reference's house pattern, /root/reference/genomeGraph/routines.go:12-65): concurrent calls with
 * equal parameters are combined into one device batch by whichever caller holds the library's lock; each caller still gets the
 * result, return code and error text of its own pair. */
int gnx_align_pair(const gnx_params *p, const uint8_t *alpha, int64_t n, const uint8_t *beta, int64_t m,
                   int64_t *out_score, gnx_cigar **out_ops, int64_t *out_n_ops);

/* ---- device-resident entry point (bench.py, multi-GPU shards) ------------------------------------ */
/* All d_* pointers are device memory on the bound device; h_* are host copies of the window tables used
 * for planning.  Kernels are enqueued on `stream` (a hipStream_t, may be NULL) and the call returns
 * after they finished.  d_ops has room for ops_capacity elements; *out_total_ops receives the number
 * used (GNX_ECAPACITY if it did not fit).
 * Contract (tests/test_device_entry_gpu.py): everything that reads the inputs or writes the outputs is queued on
 * `stream` and on nothing else, so "same stream" orders the call behind the caller's earlier work; on return the outputs are final
 * for any stream.  With GNX_ECAPACITY *out_total_ops is the need of the WHOLE batch, exactly (a second call with that capacity
 * succeeds), nothing is written at or behind d_ops[ops_capacity] in either case, and the refused call leaves no state behind.  What
 * d_score and d_ops_off hold after a refusal is UNSPECIFIED (most routes have written every score and offset, the mixed-batch route
 * neither).  The base pointers need no alignment; windows may overlap, repeat and come in any order; d_*_len and out_total_ops may
 * be NULL, d_ops may not; n_pairs == 0 writes d_ops_off[0] = 0 and nothing else. */
int gnx_align_batch_device(const gnx_params *p, int64_t n_pairs,
                           const uint8_t *d_alpha_buf, const int64_t *d_alpha_start, const int64_t *d_alpha_len,
                           const uint8_t *d_beta_buf, const int64_t *d_beta_start, const int64_t *d_beta_len,
                           const int64_t *h_alpha_len, const int64_t *h_beta_len,
                           int64_t *d_score, gnx_cigar *d_ops, int64_t ops_capacity, int64_t *d_ops_off,
                           int64_t *out_total_ops, void *stream);

/* ---- score-only entries (an extension: no Go signature of the reference returns a score alone) --------------------------------- */
/* Mirrors of gnx_align_batch / _windows / _by_offset / _device minus the CIGAR outputs: same argument conventions, same validation and
 * the same return codes for the same inputs (GNX_EBASE, GNX_EEMPTY in the low-memory modes, GNX_EINVAL, GNX_EDEVICE without a device:
 * no CPU fallback).  Contract: out_score[p] equals, for every gnx_mode, the score gnx_align_batch returns for that pair with the same
 * gnx_params (checkersize_* have no influence on it: the reference computes the score as a step of its own, highestScore_affineGap,
 * align/affineGap.go:151-207, highestScore, align/constGap.go:129-176).  All five modes are accepted; a score call never
 * returns GNX_ERANGE.  What a caller saves: checkpoints, direction matrices, snapshots, the walk and 16 bytes per CIGAR run of D2H --
 * a score needs O(n + m) state per pair and 8 bytes back.
 * Routes (gnx_timing.fast_path tells which ran): the score-only sweep (7) serves global affine and global constant gap
 * (GNX_AFFINE_GAP, GNX_CONST_GAP and their _HIGHMEM twins) with gapOpen <= 0 when every pair of the (sub-)batch has both sequences
 * non-empty, the shorter one at most 10 240 bases, and the static bound (n + m + 2) * 2 * max|penalty| below 2^30, with matrix
 * entries s - 2 * gapExtend (constant gap: s - 2 * gapPen) and gapOpen inside +-16 000; beta from plain bytes or the packed resident
 * reference.  GNX_AFFINE_GAP_LOCAL (alpha = target, beta = query, as in gnx_align_batch) takes the local variant of the sweep (8)
 * under the conditions listed at gnx_locate_batch below.  Everything else -- gapOpen > 0, a local call with gapExtend > 0, empty
 * sequences in the high-memory modes, pairs beyond those
 * bounds -- runs the route gnx_align_batch would take, and its CIGAR is dropped on the device before anything is copied back.
 * Multi-context calls (gnx_init_devices) shard and gather like the align entries; only the score vector comes back. */
int gnx_score_batch(const gnx_params *p, int64_t n_pairs, const uint8_t *alpha_cat, const int64_t *alpha_off,
                    const uint8_t *beta_cat, const int64_t *beta_off, int64_t *out_score);
int gnx_score_batch_windows(const gnx_params *p, int64_t n_pairs,
                            const uint8_t *alpha_buf, int64_t alpha_buf_len, const int64_t *alpha_start, const int64_t *alpha_len,
                            const uint8_t *beta_buf, int64_t beta_buf_len, const int64_t *beta_start, const int64_t *beta_len, int64_t *out_score);
/* beta = windows of the resident reference (gnx_set_reference; read packed, 2 bits per base) */
int gnx_score_batch_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *alpha_cat, const int64_t *alpha_off,
                              const int64_t *ref_start, const int64_t *ref_len, int64_t *out_score);
/* device-resident twin of gnx_align_batch_device: d_score[n_pairs] is device memory, the call returns after the kernels finished.
 * The same contract: queued on `stream` alone, d_score final on return and equal to the d_score of gnx_align_batch_device on the same
 * arguments, nothing written behind d_score[n_pairs]; off the sweep (routes 7 / 8) it runs the align entry's route into a CIGAR buffer
 * of the context's own, so it never returns GNX_ECAPACITY.  n_pairs == 0 is GNX_OK and writes nothing. */
int gnx_score_batch_device(const gnx_params *p, int64_t n_pairs,
                           const uint8_t *d_alpha_buf, const int64_t *d_alpha_start, const int64_t *d_alpha_len,
                           const uint8_t *d_beta_buf, const int64_t *d_beta_start, const int64_t *d_beta_len,
                           const int64_t *h_alpha_len, const int64_t *h_beta_len, int64_t *d_score, void *stream);

/* ---- locate entries: AffineGapLocal's score and the target END of its alignment, without a CIGAR (an extension, no Go signature) -- */
/* Arguments are named by ROLE: the query is aligned end to end, the target's ends are free (AffineGapLocal(target, query); the
 * reference's "150bp sequencing read to a 1kb reference sequence").  p->mode must be GNX_AFFINE_GAP_LOCAL (else GNX_EINVAL); both
 * out_score[n_pairs] and out_target_end[n_pairs] are required.  p->scores stays scores[target * 5 + query].
 * Contract: out_score[p] equals the score gnx_align_batch returns for AffineGapLocal(target, query); out_target_end[p] equals
 * len(target) minus the run length of that CIGAR's trailing GNX_COL_D run (0 if it does not end in one): the target position just
 * after the last aligned column.  An empty query gives end 0.  Validation and error codes are those of the align twin (GNX_EBASE,
 * GNX_EINVAL, GNX_EDEVICE); never GNX_ERANGE; no CPU fallback.
 * Routes: the local score sweep (gnx_timing.fast_path == 8) when gapOpen <= 0 and gapExtend <= 0, every pair of the (sub-)batch has
 * both sequences non-empty, the QUERY is at most 10 240 bases (the target may have any length, also shorter than the query),
 * s - 2 * gapExtend, -2 * gapExtend and gapOpen are inside +-16 000 and (n + m + 2) * 2 * max|penalty| is below 2^30; GNX_SCORE_SWEEP=0
 * switches it off.  Everything else runs the route gnx_align_batch takes, and a small kernel reads the end off the CIGAR on the
 * device: the end is defined identically on every route.  Multi-context calls shard and gather both vectors. */
int gnx_locate_batch(const gnx_params *p, int64_t n_pairs, const uint8_t *target_cat, const int64_t *target_off,
                     const uint8_t *query_cat, const int64_t *query_off, int64_t *out_score, int64_t *out_target_end);
int gnx_locate_batch_windows(const gnx_params *p, int64_t n_pairs,
                             const uint8_t *target_buf, int64_t target_buf_len, const int64_t *target_start, const int64_t *target_len,
                             const uint8_t *query_buf, int64_t query_buf_len, const int64_t *query_start, const int64_t *query_len,
                             int64_t *out_score, int64_t *out_target_end);
/* The read-mapping case: the TARGET is the window (ref_start[p], ref_len[p]) of the resident reference (gnx_set_reference; read
 * packed, 2 bits per base), the reads are the QUERIES.  Mind that gnx_align_batch_by_offset with GNX_AFFINE_GAP_LOCAL has the roles
 * the other way round (its alpha, the reads, is the target there). */
int gnx_locate_batch_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *query_cat, const int64_t *query_off,
                               const int64_t *ref_start, const int64_t *ref_len, int64_t *out_score, int64_t *out_target_end);

/* ---- span entries: score, target START and target end of AffineGapLocal's alignment, without a CIGAR (an extension, no Go signature) -- */
/* The arguments of the gnx_locate_* twins plus out_target_start[n_pairs]; all three output vectors are required (a null one:
 * GNX_EINVAL).  p->mode must be GNX_AFFINE_GAP_LOCAL (else GNX_EINVAL).
 * Contract: out_score and out_target_end are exactly what the locate twin returns.  out_target_start[p] is the run length of the leading
 * GNX_COL_D run of the CIGAR gnx_align_batch returns for AffineGapLocal(target, query), or 0 when the CIGAR does not begin with one:
 * the leftmost target position of the alignment (SAM POS - 1, BED chromStart), relative to the pair's own target -- also for
 * _by_offset: the caller adds ref_start[p].  A CIGAR that is a single GNX_COL_D run (an empty query) gives start = end = 0; an empty
 * target gives 0 / 0; otherwise start <= end.  Validation and return codes are the locate twins': GNX_EBASE and GNX_EINVAL are
 * reported before any output is written, GNX_EDEVICE without a device comes after the argument checks, never GNX_ERANGE.
 * Routes: under the local sweep's conditions (the list at gnx_locate_batch; GNX_SCORE_SWEEP=0 switches it off) the sweep runs
 * unchanged and a second kernel behind it, with no host round trip in between, repeats the three-state recurrence over the short
 * stretch target[lo : end] that must hold the route, carrying per state the target row where its path left column 0
 * (gnx_timing.fast_path == 10).  It compares its own score with the sweep's; a difference -- the impossible case -- returns
 * GNX_ETRACE, never a wrong start.  Route 10 serves every query the sweep serves: up to 10 240 bases.  Queries of more than 192 bases
 * hand rows over in device memory sized by the window bound, per resident wave; with gapExtend == 0 (no bound but the target itself)
 * a sub-batch whose rows would exceed 256 MB takes the fallback.  Everything else -- gapOpen > 0, gapExtend > 0, an empty sequence,
 * bounds exceeded, GNX_SCORE_SWEEP=0 -- runs the route gnx_align_batch takes and a small kernel reads both positions off the CIGAR on
 * the device: start and end are defined identically on every route.  Multi-context calls shard and gather all three vectors. */
int gnx_locate_span_batch(const gnx_params *p, int64_t n_pairs, const uint8_t *target_cat, const int64_t *target_off,
                          const uint8_t *query_cat, const int64_t *query_off, int64_t *out_score, int64_t *out_target_start, int64_t *out_target_end);
int gnx_locate_span_batch_windows(const gnx_params *p, int64_t n_pairs,
                                  const uint8_t *target_buf, int64_t target_buf_len, const int64_t *target_start, const int64_t *target_len,
                                  const uint8_t *query_buf, int64_t query_buf_len, const int64_t *query_start, const int64_t *query_len,
                                  int64_t *out_score, int64_t *out_target_start, int64_t *out_target_end);
/* target = the window (ref_start[p], ref_len[p]) of the resident reference, queries = the reads (as gnx_locate_batch_by_offset) */
int gnx_locate_span_batch_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *query_cat, const int64_t *query_off,
                                    const int64_t *ref_start, const int64_t *ref_len, int64_t *out_score, int64_t *out_target_start, int64_t *out_target_end);

/* ---- best of K on both strands: what mapping a read needs (an extension, no Go signature) ----------------------------------------- */
/* Score a read against a handful of candidate windows on either strand, keep the best, produce a CIGAR for that one only and report
 * every candidate's score.  Reads: read_cat / read_off[n_reads + 1].  Candidates of read r: cand_off[r] .. cand_off[r + 1]
 * (cand_off[0] = 0, cand_off[n_reads] = n_cand); candidate c = the window (cand_start[c], cand_len[c]) and cand_strand[c] (0: the read
 * as given, 1: its reverse complement).  _by_offset takes its windows from the resident reference (gnx_set_reference, read packed),
 * _windows from target_buf.  The reads are uploaded once; reverse complements, the selection and the winners' tables are made on the
 * device, and between the two stages only out_best (4 bytes per read) comes back -- the host plans the CIGAR stage from it.
 * Roles, by meaning and the same in both entries (p->scores is indexed [alpha * 5 + beta] as everywhere):
 *   the four global modes:   alpha = the read or its reverse complement, beta = the window;
 *   GNX_AFFINE_GAP_LOCAL:    target (alpha) = the window, query (beta) = the read or its reverse complement -- the mapping mode; mind
 *                            that gnx_align_batch_by_offset has these two the other way round.
 * Reverse complement: the read reversed with A <-> T and C <-> G; N stays N; a byte >= 5 stays a byte >= 5 and still yields GNX_EBASE
 * (dna.ReverseComplement, /root/reference/dna/modify.go:111, on upper-case bases).
 * Contract: every output equals what an existing entry returns on the flattened pair list.
 *   out_cand_score[c] (may be NULL)  global modes: what gnx_score_batch_windows / _by_offset returns for candidate c's pair; local mode:
 *                        the score gnx_locate_batch_windows / _by_offset returns for it.
 *   out_best[r]          index within read r's candidates of the FIRST maximum in candidate order (ties go to the lowest index).  A read
 *                        without candidates gets out_best = -1, score 0, target end 0 and an empty CIGAR: not an error.
 *   out_score[r], CIGAR  what gnx_align_batch_windows returns for the winning pair under the roles above (local mode on the resident
 *                        reference: alpha = the window's bases), reference quirks included, checkersize_* honoured.  *out_ops /
 *                        (*out_ops_off)[n_reads + 1] as in gnx_align_batch (gnx_free).  out_ops = out_ops_off = NULL: no CIGAR stage,
 *                        out_score[r] is the winner's candidate score (the same number).
 *   out_target_end[r] (may be NULL)  GNX_AFFINE_GAP_LOCAL only: what the locate twin returns for the winner; non-NULL in another mode:
 *                        GNX_EINVAL.
 * Return codes are those of the twins on the flattened list; GNX_EBASE or GNX_EEMPTY in ANY candidate pair, winner or not, fails the call
 * before any output is written.  GNX_EINVAL also for: cand_off not starting at 0 or decreasing (read_off decreasing), a strand byte > 1,
 * a window outside the buffer or the reference, exactly one of out_ops / out_ops_off NULL.  Never GNX_ERANGE.  Without a device:
 * GNX_EDEVICE, after the argument checks (no CPU fallback).  n_reads == 0 or n_cand == 0: GNX_OK.
 * Routes: the score stage takes the twins' routes under the twins' conditions (the score sweep, gnx_timing.fast_path 7 / 8;
 * GNX_SCORE_SWEEP=0 and everything the sweep does not take: the align route with its CIGAR left on the device); the CIGAR stage is the
 * align driver on the winners (local mode on the resident reference unpacks the winners' windows only).  Both stages are cut into
 * sub-batches of GNX_HOST_SUB pairs; a read's candidates may straddle a cut.  The call runs on context 0 alone, also after
 * gnx_init_devices (same results; the other contexts idle).  gnx_get_timing afterwards describes the score stage (fast_path,
 * fill_ms, dominant_ms, cells = candidate cells); total_ms (device) and host_ms (wall clock) cover both stages. */
int gnx_best_of_by_offset(const gnx_params *p, int64_t n_reads, const uint8_t *read_cat, const int64_t *read_off,
                          const int64_t *cand_off, const int64_t *cand_start, const int64_t *cand_len, const uint8_t *cand_strand,
                          int32_t *out_best, int64_t *out_score, int64_t *out_target_end, int64_t *out_cand_score,
                          gnx_cigar **out_ops, int64_t **out_ops_off);
int gnx_best_of_windows(const gnx_params *p, int64_t n_reads, const uint8_t *read_cat, const int64_t *read_off,
                        const uint8_t *target_buf, int64_t target_buf_len,
                        const int64_t *cand_off, const int64_t *cand_start, const int64_t *cand_len, const uint8_t *cand_strand,
                        int32_t *out_best, int64_t *out_score, int64_t *out_target_end, int64_t *out_cand_score,
                        gnx_cigar **out_ops, int64_t **out_ops_off);

/* ---- best proper pair: the two mates of a read pair placed together (an extension; the graph path has it as gnx_gsw_map_reads(paired)) -- */
typedef struct gnx_pair_opts {
    int64_t min_insert, max_insert;   /* 0 <= min_insert <= max_insert */
    int64_t unpaired_penalty;         /* >= 0 */
    int64_t _reserved;
} gnx_pair_opts;
/* gnx_best_of_* for mate pairs: reads 2k and 2k + 1 are the mates of pair k (the convention of gnx_gsw_map_reads), so n_reads is even.
 * Read and candidate tables, roles and the reverse complement are exactly those of gnx_best_of_*.  p->mode must be GNX_AFFINE_GAP_LOCAL:
 * positions are defined nowhere else.
 * Outputs: per read (n_reads) out_best, out_score, out_target_start, out_target_end (required) and out_second_score (may be NULL); per pair
 * (n_reads / 2) out_proper and out_tlen (required); per candidate out_cand_score / _start / _end (each may be NULL); out_ops / out_ops_off
 * together or both NULL, as in gnx_best_of_*.
 * Contract: every value is defined by an existing entry plus the selection rule below.
 *   out_cand_score / _start / _end[c]  what gnx_locate_span_batch_windows (_by_offset on the resident reference) returns for candidate c's
 *                        pair: target = the window, query = the read or its reverse complement; positions relative to the window.
 *   Absolute positions   A(c) = cand_start[c] + start(c), E(c) = cand_start[c] + end(c).
 *   Proper               a combination (c1, c2) of a candidate of mate 1 and one of mate 2 is proper iff their strands differ, both
 *                        alignments are non-empty (end > start) and, with f the strand-0 one and v the strand-1 one, A(f) <= A(v),
 *                        E(f) <= E(v) and min_insert <= E(v) - A(f) <= max_insert.  Its pair score is score(c1) + score(c2).
 *   Selection            P = the maximum pair score over the proper combinations, ties to the lowest c1, then the lowest c2;
 *                        U = firstmax(mate 1) + firstmax(mate 2) - unpaired_penalty, firstmax being gnx_best_of_*'s rule.  A proper
 *                        combination exists and P >= U: the mates get that combination, out_proper[k] = 1, out_tlen[k] = E(v) - A(f).
 *                        Otherwise each mate gets its own first maximum, out_proper[k] = 0, out_tlen[k] = 0.  A mate without candidates
 *                        gets -1 / 0 / 0 / 0 and an empty CIGAR, and its partner is placed alone: not an error.
 *   out_second_score[r]  the highest score among read r's candidates other than the chosen one, INT64_MIN when there is none: with
 *                        out_score[r] the input of gnx_mapq_batch.
 *   out_score[r], CIGAR  what gnx_align_batch_windows returns for the chosen pair under gnx_best_of_*'s local roles, quirks included,
 *                        checkersize_* honoured; without a CIGAR stage out_score[r] is the chosen candidate's score.
 *   out_target_start / _end[r]  the chosen candidate's span values, relative to its window: the CIGAR's leading GNX_COL_D run and the
 *                        target length minus its trailing GNX_COL_D run.
 * Return codes are those of gnx_best_of_*, all before any output is written: GNX_EBASE in ANY candidate pair fails the call; GNX_EINVAL
 * also for an odd n_reads, an option outside its range, another mode, a null required output; GNX_EDEVICE without a device, after the
 * argument checks; GNX_ETRACE is passed through from the span stage; never GNX_ERANGE; n_reads == 0: GNX_OK.
 * Routes: gnx_best_of_*'s body.  The score stage asks for the target start as well (gnx_timing.fast_path 10 under the sweep's conditions,
 * else the align route with both positions read off the CIGAR on the device); pair_select_kernel (one wave per pair, the K1 * K2
 * combinations strided over its lanes, no limit on K1 or K2) stands where the first-maximum kernel stands; the CIGAR stage is the same.
 * The result does not depend on launch geometry or sub-batch cuts.  The call runs on context 0; gnx_get_timing describes the score stage. */
int gnx_best_pair_by_offset(const gnx_params *p, const gnx_pair_opts *o, int64_t n_reads, const uint8_t *read_cat, const int64_t *read_off,
                            const int64_t *cand_off, const int64_t *cand_start, const int64_t *cand_len, const uint8_t *cand_strand,
                            int32_t *out_best, int64_t *out_score, int64_t *out_target_start, int64_t *out_target_end,
                            int64_t *out_second_score, uint8_t *out_proper, int64_t *out_tlen,
                            int64_t *out_cand_score, int64_t *out_cand_start, int64_t *out_cand_end,
                            gnx_cigar **out_ops, int64_t **out_ops_off);
int gnx_best_pair_windows(const gnx_params *p, const gnx_pair_opts *o, int64_t n_reads, const uint8_t *read_cat, const int64_t *read_off,
                          const uint8_t *target_buf, int64_t target_buf_len,
                          const int64_t *cand_off, const int64_t *cand_start, const int64_t *cand_len, const uint8_t *cand_strand,
                          int32_t *out_best, int64_t *out_score, int64_t *out_target_start, int64_t *out_target_end,
                          int64_t *out_second_score, uint8_t *out_proper, int64_t *out_tlen,
                          int64_t *out_cand_score, int64_t *out_cand_start, int64_t *out_cand_end,
                          gnx_cigar **out_ops, int64_t **out_ops_off);

/* ---- candidate windows for gnx_best_of_by_offset: a k-mer index of the resident reference and seed votes (an extension, no Go signature) -- */
/* Index of the resident reference (gnx_set_reference / _synthetic), built on the device from the packed words and kept there, on context 0.
 * 8 <= seed_len <= 32 and seed_step >= 1, else GNX_EINVAL; no resident reference: GNX_EINVAL (a reference of 0 bases is none).  Positions
 * p = 0, seed_step, 2 * seed_step, ... with p + seed_len <= len; key = the 2-bit code of ref[p .. p + seed_len), first base most significant
 * (dnaToNumber, /root/reference/genomeGraph/align.go:170); a k-mer that touches a base that is not A C G T (N, a byte >= 5) is skipped.  Two
 * device arrays sorted by key, equal keys in ascending position, positions 64-bit (16 bytes per k-mer), and a directory of first entries by
 * key prefix beside them (about one entry per k-mer, 128 MB at the most).  The index belongs to the reference: gnx_set_reference (also
 * with len = 0), gnx_set_reference_synthetic and gnx_shutdown drop it, a second build replaces the first; a failed build (GNX_ENOMEM) leaves
 * none.  It shares nothing with the graph aligner's seed index (gnx_seed_index_*) or its generation.  GNX_REF_INDEX_SUB=<positions> (read per
 * call) sets how many positions one compaction pass takes (default 2^24). */
int gnx_reference_index_build(int seed_len, int seed_step);
/* What is built (every pointer may be NULL): k-mers, bytes of device memory, the build's arguments.  No index: GNX_EINVAL. */
int gnx_reference_index_info(int64_t *out_n_kmers, int64_t *out_device_bytes, int *out_seed_len, int *out_seed_step);
/* A host copy of the index (tests, debugging): malloc'd, gnx_free.  No index: GNX_EINVAL. */
int gnx_reference_index_get(uint64_t **out_keys, uint64_t **out_pos, int64_t *out_n);

typedef struct gnx_seed_vote_opts {
    int32_t max_occ;    /* a k-mer with more index entries than this is ignored (repeats); >= 1 */
    int32_t bin;        /* width of a diagonal bin in bases; >= 8 */
    int32_t pad;        /* bases added on either side of a bin's window; >= 0 */
    int32_t max_cand;   /* candidates kept per read, 1 .. 64 */
    int32_t min_votes;  /* a bin with fewer votes is no candidate; >= 1 */
    int32_t _reserved[3];
} gnx_seed_vote_opts;
/* Reads in, the candidate tables of gnx_best_of_by_offset out.  k = the index's seed length, L = the length of the resident reference.
 * Contract, per read r of n bases and strand s (0: x = the read; 1: x = its reverse complement as gnx_best_of_* defines it):
 *   for every q in 0 .. n - k with x[q .. q + k) all A C G T: occ = the number of index entries of its code; occ == 0 or occ > max_occ: nothing;
 *   else every entry's position t casts one vote for (s, b), b = floor((t - q) / bin) -- floor, not truncation: t - q goes down to -(n - k).
 *   Candidates = the (s, b) with votes >= min_votes, ordered by votes descending, then strand ascending, then b ascending; the first max_cand
 *   are kept.  Candidate (s, b): start = clamp(b * bin - pad, 0, L), end = clamp((b + 1) * bin + n + pad, 0, L), len = end - start (>= k),
 *   strand = s.  A read shorter than k, or without a surviving bin, has no candidates.
 * Outputs (malloc'd, gnx_free): (*out_cand_off)[n_reads + 1] starting at 0, and per candidate start, len, strand -- the layout of
 * gnx_best_of_by_offset's inputs -- and votes.  The result does not depend on launch geometry, sub-batch cuts or execution order.
 * Return codes, all before any output is written: GNX_EINVAL for a null pointer, a negative count, a decreasing read_off, an option outside
 * its range, more than 2^30 diagonal bins ((L + n) / bin), or no index built; GNX_EBASE for a byte >= 5 in any read; GNX_EDEVICE without a
 * device, after the argument checks; GNX_ENOMEM when a vote table does not fit; n_reads == 0: GNX_OK with cand_off = {0}.  Never GNX_ERANGE.
 * Runs on context 0.  The vote table of a read lives in LDS (up to 512 hits) or in a slab of device memory; launches are cut by total hits
 * so that the slabs stay inside the workspace limit of gnx_init.  Switches, read per call: GNX_SEED_VOTE_LDS=0 sends every read to the slab
 * form; GNX_SEED_SUB=<hits> sets the hits per vote launch.  gnx_get_timing afterwards: fast_path 11. */
int gnx_seed_candidates(const gnx_seed_vote_opts *o, int64_t n_reads, const uint8_t *read_cat, const int64_t *read_off,
                        int64_t **out_cand_off, int64_t **out_cand_start, int64_t **out_cand_len, uint8_t **out_cand_strand, int32_t **out_cand_votes);

/* ---- alignment summaries: what is IN a finished alignment (an extension; the reference's notion is scoreAffineAln, ------------------- */
/* align/affineGap_highMem.go:355-385: a score computed from the columns of an alignment) */
#define GNX_XCOL_EQ 3   /* extended CIGAR only: an M column whose two bases are the same byte  ('=') */
#define GNX_XCOL_X  4   /* extended CIGAR only: an M column whose two bases differ             ('X') */
typedef struct gnx_aln_summary {      /* 12 x int64 = 96 bytes */
    int64_t rescore;
    int64_t alpha_used, beta_used;
    int64_t alpha_start, alpha_end;
    int64_t n_equal, n_mismatch;
    int64_t ins_bases, del_bases;
    int64_t gap_runs;
    int64_t n_xops;
    int64_t _reserved;                /* 0 */
} gnx_aln_summary;
/* Walk the CIGARs of a batch against their sequences on the device: identities and substitutions, edit distance, the column re-score,
 * the =/X form of the CIGAR.  Sequences as in gnx_align_batch / _windows; ops / ops_off[n_pairs + 1] in the layout the align entries
 * return.  out[n_pairs] is required.  out_xops / out_xops_off are given together or both NULL (no extended CIGAR is produced); when
 * given they are malloc'd (gnx_free) in the layout of out_ops / out_ops_off.
 * _by_offset has the roles of gnx_best_of_by_offset, whose CIGARs it exists for: the four global modes alpha = the read, beta = the
 * window of the resident reference; GNX_AFFINE_GAP_LOCAL alpha (target) = the window, beta (query) = the read.  The caller passes each
 * read in the orientation it was aligned in (a strand-1 winner as its reverse complement).
 * Everything is a function of the pair's COLUMN SEQUENCE: the CIGAR expanded run by run into M / I / D columns.  Runs of length 0
 * contribute nothing, so adjacent runs of one op are one run.  The sequence is anchored at (0, 0): an M column consumes alpha[i] and
 * beta[j], I consumes beta[j] only, D alpha[i] only (align/view.go:47-55).
 *   alpha_used, beta_used   bases consumed; may be fewer than the sequences hold (quirk Q2 produces such CIGARs; a caller who wants
 *                           one anchored at the end passes shifted windows).
 *   n_equal / n_mismatch    M columns with alpha[i] == beta[j] as bytes (N against N is equal) / the others.
 *   charged columns         GNX_AFFINE_GAP_LOCAL: the leading maximal D run and the trailing maximal D run of the column sequence are
 *                           free (freeEndGaps, affineGap_highMem.go:188-210); a sequence that is one D run is free as a whole.  In
 *                           every other mode nothing is free.
 *   ins_bases / del_bases   charged I / D columns.
 *   gap_runs                maximal runs of equal gap op among the charged columns (an I run directly followed by a D run: two).
 *   alpha_start, alpha_end  local mode: the length of the free leading run, and alpha_used minus the free trailing run (one free run
 *                           as a whole: 0 / 0, as gnx_locate_span_* defines it); other modes: 0 and alpha_used.
 *   rescore                 the sum of scores[alpha[i] * 5 + beta[j]] over the M columns, plus -- affine modes (0, 2, 3) --
 *                           gap_open * gap_runs + gap_extend * (ins_bases + del_bases) (scoreAffineAln's rule), or -- constant-gap
 *                           modes (1, 4) -- gap_open * (ins_bases + del_bases).  checkersize_* are ignored.
 *   extended CIGAR          the maximal runs of the column sequence with every M column retyped GNX_XCOL_EQ or GNX_XCOL_X; I = 1 and
 *                           D = 2 are kept, free D runs included.  n_xops = the number of those runs, also without out_xops.
 * Return codes, all before any output is written: GNX_EINVAL for a null required pointer, a negative count, an unknown mode, ops_off
 * not starting at 0 or decreasing, an op > 2, a negative run length, a CIGAR that consumes more than its alpha or beta holds, exactly
 * one of out_xops / out_xops_off NULL, a window outside its buffer or the reference, a sequence of 2^30 bases or more (the limit of the
 * align entries); GNX_EBASE exactly where the align twin reports it
 * for the same sequences (a byte >= 5 anywhere in either); GNX_EDEVICE without a device, after the argument checks (no CPU fallback);
 * n_pairs == 0: GNX_OK; never GNX_ERANGE.
 * Runs on context 0.  aln_summary_kernel (aln_summary.hip.h): one wave per pair, the CIGAR in blocks of 64 runs, long M runs 64 columns
 * per step, the packed reference read in place.  Calls are cut into launches of GNX_HOST_SUB pairs.  Switches, read per call:
 * GNX_SUMMARY_SUB=<pairs> overrides that cut; GNX_SUMMARY_FORM=0 / 1 walks every M run a lane per column / a lane per run (same results).
 * gnx_get_timing afterwards: fast_path 12. */
int gnx_summarize_batch(const gnx_params *p, int64_t n_pairs,
                        const uint8_t *alpha_cat, const int64_t *alpha_off, const uint8_t *beta_cat, const int64_t *beta_off,
                        const gnx_cigar *ops, const int64_t *ops_off,
                        gnx_aln_summary *out, gnx_cigar **out_xops, int64_t **out_xops_off);
int gnx_summarize_batch_windows(const gnx_params *p, int64_t n_pairs,
                                const uint8_t *alpha_buf, int64_t alpha_buf_len, const int64_t *alpha_start, const int64_t *alpha_len,
                                const uint8_t *beta_buf, int64_t beta_buf_len, const int64_t *beta_start, const int64_t *beta_len,
                                const gnx_cigar *ops, const int64_t *ops_off,
                                gnx_aln_summary *out, gnx_cigar **out_xops, int64_t **out_xops_off);
int gnx_summarize_batch_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *read_cat, const int64_t *read_off,
                                  const int64_t *ref_start, const int64_t *ref_len,
                                  const gnx_cigar *ops, const int64_t *ops_off,
                                  gnx_aln_summary *out, gnx_cigar **out_xops, int64_t **out_xops_off);

/* ---- MD strings: the reference letters of a finished alignment (an extension; SAM's MD:Z tag) -------------------------------------- */
/* The MD string of every pair of a batch, written on the device: the resident reference exists there only (2 bits per base), so
 * nothing else can name the reference base under a substitution or a deletion.  Sequences, ops and ops_off as in the gnx_summarize_*
 * twin.  Outputs, both required, malloc'd (gnx_free): *out_md = the strings' bytes one behind the other, no terminators;
 * (*out_md_off)[n_pairs + 1], starting at 0: pair k's string is (*out_md)[off[k] .. off[k + 1]).
 * Contract.  Everything is a function of the pair's column sequence as gnx_summarize_* defines it (runs of length 0 vanish, adjacent equal
 * ops are one run, anchored at (0, 0)).  ALPHA IS THE DESCRIBED (REFERENCE) SIDE: M and D consume it.  Letters are "ACGTN"[code]; equality is
 * equality of bytes, so N against N is equal, exactly as n_equal counts.
 *   Range   GNX_AFFINE_GAP_LOCAL: the leading maximal D run and the trailing maximal D run are outside (the free end gaps, the columns
 *           the summary un-charges); a sequence that is one D run has nothing inside.  Every other mode: all columns are inside.
 *   Walk    the inside columns in order with a counter run = 0:
 *             M, equal bytes       run += 1
 *             M, different bytes   emit dec(run), the alpha letter; run = 0
 *             I                    nothing: the counter runs on across it
 *             D whose previous COLUMN (an I column counts) is not an inside D column    emit dec(run), '^', the alpha letter; run = 0
 *             D directly behind an inside D column                                      emit the alpha letter only
 *           and at the end emit dec(run).
 * Every string matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*; an alignment with nothing inside gives "0".  The numbers sum to the summary's
 * n_equal, the letters outside ^ groups number n_mismatch, the letters inside ^ groups number del_bases.
 * E.g. alpha ACGTACGTAC, beta ACGAACTAC, 6M 1D 3M: "3T2^G3"; beta TTTACG, 3D 2I 4M 3D: "4" in GNX_AFFINE_GAP_LOCAL, "0^ACG4^TAC0" elsewhere.
 * gnx_md_batch and _windows take all five modes.  _by_offset takes GNX_AFFINE_GAP_LOCAL only: there the window of the resident reference
 * is alpha, while in the global modes _by_offset makes the read alpha and the string would spell the read; any other mode is GNX_EINVAL
 * (gnx_best_pair_*'s rule).
 * Return codes are the summary twin's, all before any output is written: GNX_EINVAL for a null required pointer (out_md and out_md_off
 * included), a negative count, an unknown mode, ops_off not starting at 0 or decreasing, an op > 2, a negative run length, a CIGAR that
 * consumes more than its alpha or beta holds, a window outside its buffer or the reference, a sequence of 2^30 bases or more; GNX_EBASE
 * exactly where the align twin reports it (a byte >= 5 anywhere in either sequence); GNX_EDEVICE without a device, after the argument
 * checks (no CPU fallback); n_pairs == 0: GNX_OK with off = {0}; never GNX_ERANGE.
 * Runs on context 0.  aln_md_kernel (aln_md.hip.h) has aln_summary_kernel's geometry; a first instantiation counts each pair's bytes, the
 * scan family turns the counts into offsets, a second one writes.  Calls are cut into launches of GNX_HOST_SUB pairs.  Switches, read per
 * call: GNX_MD_SUB=<pairs> overrides that cut; GNX_MD_FORM=0 / 1 walks every M and D run a lane per column / a lane per run (same bytes).
 * gnx_get_timing afterwards: fast_path 13. */
int gnx_md_batch(const gnx_params *p, int64_t n_pairs,
                 const uint8_t *alpha_cat, const int64_t *alpha_off, const uint8_t *beta_cat, const int64_t *beta_off,
                 const gnx_cigar *ops, const int64_t *ops_off, char **out_md, int64_t **out_md_off);
int gnx_md_batch_windows(const gnx_params *p, int64_t n_pairs,
                         const uint8_t *alpha_buf, int64_t alpha_buf_len, const int64_t *alpha_start, const int64_t *alpha_len,
                         const uint8_t *beta_buf, int64_t beta_buf_len, const int64_t *beta_start, const int64_t *beta_len,
                         const gnx_cigar *ops, const int64_t *ops_off, char **out_md, int64_t **out_md_off);
int gnx_md_batch_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *read_cat, const int64_t *read_off,
                           const int64_t *ref_start, const int64_t *ref_len,
                           const gnx_cigar *ops, const int64_t *ops_off, char **out_md, int64_t **out_md_off);
/* The MAPQ of n placements from each one's score S = score[r] and the best score among its other candidates, second_score[r] (INT64_MIN:
 * there is none -- gnx_best_pair_*'s out_second_score as it comes).  This is THIS LIBRARY's rule, not BWA's and not Bowtie's:
 *   S <= 0: 0;   s2 = second_score[r] < 0 ? 0 : second_score[r] (INT64_MIN included);   s2 >= S: 0;
 *   otherwise min(60, floor(60 * (S - s2) / S)), exact for every int64 S (the product is taken 128 bits wide).
 * E.g. (400, none) 60, (400, 200) 30, (400, 399) 0, (400, 1) 59, (61, 1) 59, (2^62, 2^61) 30.
 * Pure host arithmetic: no device, no gnx_init.  n < 0, or a null pointer with n > 0: GNX_EINVAL. */
int gnx_mapq_batch(int64_t n, const int64_t *score, const int64_t *second_score, uint8_t *out_mapq);

/* ---- Pileup: per-base counts of placed reads on the resident reference, and the calls they give (an extension; sam/pileup.go's stage) -- */
/* ONE pile per process, resident on the device beside the reference (context 0) and owned by it: gnx_set_reference[_synthetic] -- a new
 * reference or its release -- and gnx_shutdown drop the pile; gnx_reference_index_build does not.  It covers the region
 * [region_start, region_start + region_len) of the reference.  What comes back is small: rows on request (gnx_pileup_get) and the sparse
 * list of positions where the reads disagree with the reference (gnx_pileup_calls); reads, CIGARs and reference stay where they are.
 * Insertion sequences and deletion lengths are kept only by a pile that was told to track alleles (gnx_pileup_track_alleles, below; the
 * reference's Pile has maps of both); otherwise a count per position is all there is.
 *
 * gnx_pileup_add_by_offset.  GNX_AFFINE_GAP_LOCAL only (any other mode: GNX_EINVAL).  Roles, sequences, ops and ops_off are those of
 * gnx_md_batch_by_offset: the window (ref_start[k], ref_len[k]) is alpha, the read is beta in the orientation it was aligned in -- a
 * strand-1 winner is passed as its reverse complement, so every counted base is a forward-strand base; strand[k] in {0, 1} only picks the
 * counter.  Everything is a function of the pair's column sequence as gnx_summarize_* defines it (runs of length 0 vanish, adjacent equal
 * ops are one run, anchored at (0, 0)).  The leading and the trailing maximal D run are outside, so alpha_start and alpha_end are the
 * summary's; a sequence that is one D run has nothing inside.  For pair k with use == NULL or use[k] != 0, with x = ref_start[k] + i for a
 * column at alpha position i, and only where region_start <= x < region_start + region_len:
 *   an inside M column over read byte b             base[strand][b] += 1 at x (a read N counts in slot 4)
 *   an inside D column                              del[strand] += 1 at x
 *   a maximal inside I run behind i consumed alpha bases, alpha_start < i < alpha_end      ins[strand] += 1 at ref_start[k] + i - 1
 * A terminal I run (i == alpha_start or i == alpha_end) is a soft clip, as the reference's sclipTerminalIns treats it, and counts
 * nowhere.  Columns outside the region contribute nothing; a read wholly outside the region is not an error.
 * E.g. window at 100 = ACGTACGTAC, read ACGAACTAC, 6M 1D 3M, strand 0: base A at 100, C at 101, G at 102, A at 103, A at 104, C at 105, del
 * at 106, T at 107, A at 108, C at 109.  Same window, read TTTACG, 3D 2I 4M 3D: T, A, C, G at 103 .. 106 and nothing else (both D runs are
 * outside, the I run stands at i == alpha_start).
 * Return codes, all before the pile changes: those of gnx_md_batch_by_offset (GNX_EBASE exactly where that twin reports it: a byte >= 5
 * anywhere in a read, or in a window's exception blocks, used or not), and GNX_EINVAL also without an open pile, for a strand byte > 1, and
 * for a call that would carry reads_added past 2^31 - 1 (every counter grows by at most 1 per read, so int32 cannot overflow).
 * n_pairs == 0: GNX_OK; GNX_EDEVICE without a device, after the argument checks; never GNX_ERANGE.
 * pile_add_kernel (pileup.hip.h) has aln_summary_kernel's geometry and reads no reference; the counters are 14 planes of region_len int32
 * bumped with atomic adds.  Calls are cut into launches of GNX_HOST_SUB pairs.  Switches, read per call: GNX_PILE_SUB=<pairs> overrides
 * that cut; GNX_PILE_FORM=0 / 1 walks every M and D run a lane per column / a lane per run (same counts).  gnx_get_timing afterwards:
 * fast_path 14, cells = the CIGAR columns of the added pairs, dominant_ms = pile_add_kernel alone (fill_ms: with the base check).
 *
 * gnx_pileup_open: a zeroed pile over the region; an open pile is replaced.  GNX_EINVAL for region_start < 0, region_len < 1, without a
 * resident reference, for a region that leaves it; GNX_ENOMEM when the table (56 bytes per position) does not fit -- the previous pile
 * then stays as it was.  gnx_pileup_info: any pointer may be NULL; GNX_EINVAL without an open pile.  gnx_pileup_get: rows
 * region_start + first .. + count as gnx_pile; GNX_EINVAL for rows outside the region, a null `out` with count > 0, no open pile.
 * gnx_pileup_close: releases the pile; without one: GNX_OK.
 *
 * gnx_pileup_calls.  THIS LIBRARY's rule (as gnx_mapq_batch's is), not a variant caller's.  For every position x of the region, ascending,
 * with c the reference code at x (4 in an exception block): cnt[a] = base[0][a] + base[1][a], del = del[0] + del[1], ins = ins[0] + ins[1],
 * depth = cnt[0] + .. + cnt[4] + del.  c == 4: nothing is emitted at x.
 *   Primary call     the candidates are the bases a in {0, 1, 2, 3} other than c, then the deletion; the winner is the largest count, ties
 *                    going to the smaller index, the deletion last.  Emitted as kind 0 (alt = a) or kind 1 (alt = 0xFF) if
 *                    depth >= min_depth, count >= min_alt, count * frac_den >= frac_num * depth (in 64 bits) and, with both_strands, both
 *                    strand counts are at least 1.
 *   Insertion call   kind 2 (alt = 0xFF), behind x: the same four tests with count = ins against the same depth.
 * Output ordered by position, the primary call before the insertion call; ref = c, count_fwd = the strand-0 share of count.  *out_calls is
 * malloc'd (gnx_free), also for *out_n == 0.  GNX_EINVAL for min_depth < 1, min_alt < 1, not 1 <= frac_num <= frac_den <= 2^20,
 * both_strands outside {0, 1}, a null pointer, no open pile -- nothing is written then.  pile_call_kernel: one position per lane, a count
 * pass, the scan family, a write pass.  gnx_get_timing afterwards: fast_path 15, cells = the region's positions. */
typedef struct gnx_pile {            /* 16 x int32 = 64 bytes, one reference position */
    int32_t base[2][5];              /* [strand][A C G T N]: read bases in M columns over this position */
    int32_t del[2];                  /* inside D columns over this position */
    int32_t ins[2];                  /* maximal inside I runs directly behind this position */
    int32_t _reserved[2];            /* 0 */
} gnx_pile;
typedef struct gnx_pile_call_opts { int32_t min_depth, min_alt, frac_num, frac_den, both_strands, _reserved; } gnx_pile_call_opts;
typedef struct gnx_pile_call {       /* 24 bytes */
    int64_t pos;                     /* 0-based reference position */
    int32_t depth, count, count_fwd;
    uint8_t kind, ref, alt, _pad;    /* kind 0 substitution, 1 deletion, 2 insertion; alt: a base code for kind 0, else 0xFF */
} gnx_pile_call;
int gnx_pileup_open(int64_t region_start, int64_t region_len);
int gnx_pileup_info(int64_t *out_start, int64_t *out_len, int64_t *out_reads_added, int64_t *out_device_bytes);
int gnx_pileup_add_by_offset(const gnx_params *p, int64_t n_pairs, const uint8_t *read_cat, const int64_t *read_off,
                             const int64_t *ref_start, const int64_t *ref_len, const uint8_t *strand,
                             const gnx_cigar *ops, const int64_t *ops_off, const uint8_t *use /* NULL: all */);
int gnx_pileup_get(int64_t first, int64_t count, gnx_pile *out);
int gnx_pileup_calls(const gnx_pile_call_opts *o, gnx_pile_call **out_calls, int64_t *out_n);
int gnx_pileup_close(void);

/* ---- The alleles of the pile: which deletion, which insertion (the reference's Pile.DelCountF/R keyed by length at the 5'-most deleted
 * base, InsCountF/R keyed by sequence), the calls they give, and with gonomics_amd/vcf.py a VCF record for each ------------------------- */
/* gnx_pileup_track_alleles switches the open pile to tracking: every later gnx_pileup_add_by_offset also appends one event per indel to a
 * log on the device (reads and CIGARs are there only during the add).  Allowed only while reads_added == 0: GNX_EINVAL otherwise, as
 * without an open pile and for reserve_events < 0.  reserve_events sizes the first log (0: a default of 2^16 events); it is a starting
 * size, not a limit: an add grows the log, beside the old one, before its first launch that could change the pile, and a growth that
 * fails is GNX_ENOMEM with pile and log as they were.  gnx_pileup_open replaces the pile, so tracking is off again; whatever drops the
 * pile drops the log.  gnx_pileup_info keeps reporting the planes only; gnx_pileup_allele_info (any pointer may be NULL; GNX_EINVAL
 * without an open pile) gives tracking 0 / 1, the events logged so far and the log's bytes on the device (0 when not tracking).  A pile that
 * does not track behaves exactly as before: the same launches, the same bytes.
 *
 * What an add records, for pair k with use == NULL or use[k] != 0, as a function of the column sequence (see gnx_pileup_add_by_offset):
 *   Deletion    each MAXIMAL inside D run of L columns whose first column is at alpha position i: (pos = ref_start[k] + i, kind 1,
 *               length L), iff pos lies in the region -- and then whole, even if it runs past the region's end.  A run that starts before
 *               the region records nothing, though its columns inside still bump `del` (the reference: "only recorded for the 5'-most
 *               base").
 *   Insertion   each MAXIMAL inside I run of L read bases behind i consumed alpha bases with alpha_start < i < alpha_end -- the runs that
 *               bump `ins` --: pos = ref_start[k] + i - 1, iff pos lies in the region.  L <= 21: kind 2 with the bases packed into seq, 3 bits
 *               each, (code + 1), the first base in the lowest bits, a read N (code 4) as digit 5, 0 ends.  L > 21: kind 3, length only.
 *               21 bases is what 63 bits hold at 3 bits a base; kind 3 MERGES different sequences of equal length.
 * The leading and trailing D run and a terminal I run record nothing.  A maximal run may be written as several runs, with zero-length runs
 * of other ops between them: it is one event.  E.g. window at 100 = ACGTACGTAC, read ACGAACTAC, 6M 1D 3M: (pos 106, kind 1, length 1).
 * Same window, read ACGTTTACGTAC, 4M 2I 6M: (pos 103, kind 2, length 2, seq = 4 | 4 << 3 = 36).  TTTACG, 3D 2I 4M 3D: nothing.
 * Every error of the add is still raised before anything changes, the log included; more than 2^31 - 1 events in one pile: GNX_EINVAL
 * before anything changes.  An add on a tracking pile stays fast_path 14 with dominant_ms = pile_add_kernel alone; allele_log_kernel
 * (pile_alleles.hip.h: one lane per run, events appended with one atomic add per wave and block of 64 runs) runs behind it over the same
 * sub-batch cuts and counts in fill_ms.
 *
 * gnx_pileup_alleles: the distinct alleles with their counts, ordered by (pos, kind, key), key = length for kinds 1 and 3 and seq as an
 * unsigned number for kind 2.  The log's order is no part of the contract and no result depends on it; the query leaves the log as it is, so
 * it may be called twice and between adds.  Invariants: per position and strand the counts of kinds 2 + 3 sum to ins[strand] of the planes;
 * the counts of kind 1 at x never exceed del[strand] at x.  *out is malloc'd (gnx_free), also for *out_n == 0.  GNX_EINVAL for a null
 * pointer, without an open pile, without tracking.  Two stable radix sorts, a count pass, the scan family, a write pass.  gnx_get_timing:
 * fast_path 16, cells = the events.
 *
 * gnx_pileup_indel_calls: THIS LIBRARY's rule, as gnx_pileup_calls' is, with its options and its argument errors (and GNX_EINVAL without
 * tracking).  For every allele in the order above, with c the reference code at pos (c == 4: silent) and depth exactly gnx_pileup_calls'
 * depth at pos: emitted if it passes the same four tests with its own count / count_fwd.  Several alleles at one position may all pass.
 * gnx_get_timing: fast_path 17, cells = the alleles.
 *
 * gnx_pileup_alleles_norm / gnx_pileup_indel_calls_norm: the same two queries over LEFT-NORMALISED events.  The plain
 * queries leave an allele where the CIGAR puts it, so one deletion in a homopolymer or a tandem repeat comes out as several alleles with a
 * share of the count each; these move every event of the log to its leftmost placement first.  The rule is the standard one (bcftools norm;
 * Tan et al. 2015), taken per allele against the reference alone, R = the reference in codes, lo = the pile's region_start:
 *   Deletion (x, L)            while x - 1 >= lo, R[x - 1] < 4 and R[x - 1] == R[x + L - 1]: x -= 1.  The length does not change.
 *   Insertion (x, s), kind 2   while x - 1 >= lo, R[x] < 4, s's last base is no read N and R[x] == s[L - 1]: s = R[x] + s[0 .. L - 1), x -= 1.
 *   Long insertion, kind 3     unchanged: only its length was kept, and without its bases it cannot be shifted.
 * An N, in the reference or among the inserted bases, matches nothing and stops the shift.  The position never goes below region_start:
 * the result is the leftmost placement INSIDE THE REGION, so a pile whose region starts inside a repeat reports the allele at the
 * region's first base where a wider region would move it further.  The shift has no upper bound.  E.g. reference GATTTTTC: deletion (6, 1)
 * -> (2, 1); insertion T behind 6 -> T behind 1; insertion GT behind 6 -> TG behind 5.
 * The normalised events are then reduced as gnx_pileup_alleles reduces the raw ones -- alleles that stood apart may merge; the sum of count
 * and of count_fwd over the alleles of a kind equals the plain query's -- and gnx_pileup_indel_calls_norm puts them to gnx_pileup_indel_calls'
 * four tests with that rule's depth and reference code at the NORMALISED position.  Signatures, errors and the ownership of the result
 * are those of the plain entries.  The log stays raw: a plain query after a normalised one returns what it returned before, and adds go on
 * as before.  The del / ins counters of the planes, and so gnx_pileup_calls, stay per column.  gnx_get_timing: fast_path 18 (alleles) and
 * 19 (calls), dominant_ms = norm_shift_kernel alone (pile_norm.hip.h).  GNX_NORM_COOP=0 makes every lane of that kernel finish its event
 * alone; the results are the same.
 *
 * Not in scope: the sequences of insertions longer than 21 bases; normalising an allele across other variants of the same read; base
 * qualities; more than one region. */
typedef struct gnx_pile_allele {     /* 32 bytes */
    int64_t  pos;                    /* deletion: its first deleted base; insertion: the base it stands behind (0-based) */
    uint64_t seq;                    /* kind 2: the inserted bases, 3 bits each, (code + 1), first base in the lowest bits, 0 ends; else 0 */
    int32_t  length;                 /* deleted / inserted bases */
    int32_t  count, count_fwd;       /* reads with exactly this allele; the strand-0 share */
    uint8_t  kind, _pad[3];          /* 1 deletion, 2 insertion (<= 21 bases, sequence kept), 3 long insertion (> 21, sequence not kept) */
} gnx_pile_allele;
typedef struct gnx_pile_indel_call { /* 40 bytes: the allele, then what the rule saw */
    int64_t  pos;
    uint64_t seq;
    int32_t  length, count, count_fwd;
    uint8_t  kind, _pad[3];
    int32_t  depth;                  /* gnx_pileup_calls' depth at pos */
    uint8_t  ref, _pad2[3];          /* the reference code at pos */
} gnx_pile_indel_call;
int gnx_pileup_track_alleles(int64_t reserve_events);
int gnx_pileup_allele_info(int32_t *out_tracking, int64_t *out_events, int64_t *out_device_bytes);
int gnx_pileup_alleles(gnx_pile_allele **out, int64_t *out_n);
int gnx_pileup_indel_calls(const gnx_pile_call_opts *o, gnx_pile_indel_call **out_calls, int64_t *out_n);
int gnx_pileup_alleles_norm(gnx_pile_allele **out, int64_t *out_n);
int gnx_pileup_indel_calls_norm(const gnx_pile_call_opts *o, gnx_pile_indel_call **out_calls, int64_t *out_n);

/* ---- Base qualities in the pile, and diploid SNP genotypes from them ---------------------------------------------------- */
/* gnx_pileup_track_qualities switches the open pile to quality tracking: four more planes of region_len int32 beside the 14, qsum[A C G T],
 * the summed Phred qualities of the counted read bases, both strands together (16 bytes per position).  Allowed only while
 * reads_added == 0: GNX_EINVAL otherwise, as without an open pile and for min_baseq outside 0 .. 93; an allocation that fails is GNX_ENOMEM
 * with the pile as it was.  gnx_pileup_open replaces the pile, so quality tracking is off again; whatever drops the pile drops the planes.
 * It is independent of gnx_pileup_track_alleles: both may be on, in either order, and the allele log does not depend on quality (an indel
 * has none).  gnx_pileup_info keeps reporting the 14 planes; gnx_pileup_qual_info (any pointer may be NULL; GNX_EINVAL without an open
 * pile) gives tracking 0 / 1, min_baseq and the planes' bytes, 16 * region_len (a plain pile: 0, 0, 0).  A pile that does not track
 * qualities behaves exactly as before: the same launches, the same bytes.
 *
 * gnx_pileup_add_by_offset_qual: gnx_pileup_add_by_offset with one more array.  qual_cat is laid out exactly like read_cat and uses the
 * same read_off; its bytes are raw Phred values (NOT ASCII + 33) in the orientation the read is passed in -- who reverse-complements a
 * strand-1 read reverses its qualities.  A byte above 93 counts as 93 (clamped on the device; there is no error for it).  Everything
 * gnx_pileup_add_by_offset defines holds, with one change.  An inside M column over read byte b with quality q = min(byte, 93):
 *   q < min_baseq     counts nowhere (samtools' -Q)
 *   otherwise         base[strand][b] += 1 as before and, for b < 4, qsum[b] += q
 * del, ins and the allele log do not depend on quality.  Return codes are those of the plain add, all raised before the pile changes.
 * The two entries do not mix: gnx_pileup_add_by_offset on a pile that tracks qualities is GNX_EINVAL, this entry on a pile that does not
 * is GNX_EINVAL, and so is a null qual_cat with n_pairs > 0.  A read adds at most 93 to a qsum counter, so on a quality pile reads_added
 * may not pass (2^31 - 1) / 93 = 23 091 222: a call that would carry it further is GNX_EINVAL before anything changes.
 * E.g. window at 100 = ACGTACGTAC, read ACGAACTAC, 6M 1D 3M, qualities 30 30 10 30 40 30 5 30 30, min_baseq 20: the G at 102 and the T at
 * 107 count nowhere; qsum[A] = 30 at 100, 103 and 108 and 40 at 104; qsum[C] = 30 at 101, 105 and 109; del at 106 as before.
 * qual_add_kernel (pile_qual.hip.h) has pile_add_kernel's geometry, cuts and switches (GNX_PILE_SUB, GNX_PILE_FORM) and issues up to two
 * unreturned atomic adds per M column.  gnx_get_timing: fast_path 14, cells as in the plain add, dominant_ms = qual_add_kernel alone.
 *
 * gnx_pileup_get_qual: the qsum rows region_start + first .. + count as [count][4] int32, A C G T; gnx_pileup_get's argument rules, and
 * GNX_EINVAL without quality tracking.
 *
 * gnx_pileup_genotypes.  THIS LIBRARY's rule, as gnx_mapq_batch's and gnx_pileup_calls' are: a diploid SNP genotype per position from the
 * counts and the quality sums, integer only, in centi-Phred (1/100 of a Phred unit).  For every position x of the region, ascending, with
 * c the reference code at x (c == 4: silent), n[a] = base[0][a] + base[1][a] and Q[a] = qsum[a] for a in A C G T:
 *   depth = n[0] + n[1] + n[2] + n[3]           (read Ns and deletions are outside the model)
 *   E[a]  = 100 * Q[a] + 477 * n[a], in 64 bits  what it costs to explain all a bases as errors; 477 = round(1000 log10 3): a miscall
 *                                               lands on one of three letters.  The -10 log10(1 - e) term of correct bases is dropped.
 *   b     = the a != c with the largest E[a], ties to the smaller index: the alternative
 *   L[0]  = E[b]                                ref / ref
 *   L[1]  = 301 * (n[c] + n[b]) + prior_het     ref / alt; 301 = round(1000 log10 2)
 *   L[2]  = E[c] + prior_hom                    alt / alt
 * (bases of the other two letters cost every genotype the same and cancel).  g = argmin L, ties to the smaller index; pl[k] = L[k] - L[g];
 * gq = the smallest pl[k] with k != g; qual = max(0, L[0] - min(L[1], L[2])); pl, gq and qual saturate at 2^31 - 1.  A record is emitted
 * iff depth >= min_depth, g != 0 and qual >= min_qual: gt = g, ref = c, alt = b, ref_count = n[c], alt_count = n[b], alt_fwd = base[0][b].
 * E.g. prior_het 3000, prior_hom 3300: 10 ref + 10 alt bases at q30: L = (34 770, 9 020, 38 070), g = 1, qual = gq = 25 750.  19 ref +
 * 1 alt at q30: L = (3 477, 9 020, ..), g = 0, nothing is emitted.  17 ref + 3 alt at q30: L = (10 431, 9 020, 62 409), g = 1, qual 1 411.
 * Twenty q2 alt bases (E = 13 540) against ten q40 ref bases (E = 44 770) are no alt / alt call -- L[2] = 48 070 against L[0] = 13 540 --
 * where a count rule sees two thirds alt.
 * Output ordered by position; *out is malloc'd (gnx_free), also for *out_n == 0.  GNX_EINVAL for min_depth < 1, min_qual < 0, a prior
 * outside 0 .. 2^20, a null pointer, no open pile, a pile without quality tracking -- nothing is written then.  geno_call_kernel
 * (pile_qual.hip.h) has pile_call_kernel's geometry and reads 12 planes; the rule itself is geno_rule() of gonomics_amd/csrc/geno_rule.h,
 * which a CPU program can call as well.  gnx_get_timing: fast_path 20, cells = the region's positions.
 *
 * Not in scope: indel genotypes (an indel allele carries no quality; gnx_pileup_indel_calls remains the rule for them), mapping qualities
 * inside the likelihood (filter with `use`), more than two alleles in a genotype. */
typedef struct gnx_geno_opts { int32_t min_depth, min_qual, prior_het, prior_hom, _reserved[2]; } gnx_geno_opts;
typedef struct gnx_pile_genotype {   /* 48 bytes */
    int64_t pos;                     /* 0-based reference position */
    int32_t pl[3];                   /* centi-Phred, 0 for the called genotype: ref/ref, ref/alt, alt/alt */
    int32_t gq, qual;                /* centi-Phred */
    int32_t depth, ref_count, alt_count, alt_fwd;
    uint8_t gt, ref, alt, _pad;      /* gt 1 (ref / alt) or 2 (alt / alt); ref, alt: base codes; _pad 0 */
} gnx_pile_genotype;
int gnx_pileup_track_qualities(int32_t min_baseq);
int gnx_pileup_qual_info(int32_t *out_tracking, int32_t *out_min_baseq, int64_t *out_device_bytes);
int gnx_pileup_add_by_offset_qual(const gnx_params *p, int64_t n_pairs, const uint8_t *read_cat, const int64_t *read_off,
                                  const int64_t *ref_start, const int64_t *ref_len, const uint8_t *strand,
                                  const gnx_cigar *ops, const int64_t *ops_off, const uint8_t *use /* NULL: all */,
                                  const uint8_t *qual_cat);
int gnx_pileup_get_qual(int64_t first, int64_t count, int32_t *out /* [count][4]: A C G T */);
int gnx_pileup_genotypes(const gnx_geno_opts *o, gnx_pile_genotype **out, int64_t *out_n);

int gnx_get_timing(gnx_timing *out);
/* Diagnostics (tests only; nothing in the reference corresponds to it): launch n_workgroups workgroups that each hold one CU's whole
 * LDS and spin for `milliseconds` on a stream of their own, and return at once -- the pipelined launches of the library must make
 * progress whatever else occupies the device (no workgroup waits for work that has not been claimed by a running one). */
int gnx_debug_occupy(int n_workgroups, int milliseconds); /* refused with GNX_EINVAL unless the process runs with GNX_DEBUG_ENTRY=1 */
/* Diagnostics: which = 0: number of items of pipelined launches (strips, row-block levels) that were run by a workgroup other
 * than their own since the last reset -- the abnormal path of the claim protocol, which tests/test_ticket.py forces and then
 * proves to have run.  which = 1 / 2: combined batches run for concurrent gnx_align_pair calls / pairs served by them.
 * which = 3 / 4: checkerboard edges the affine walks of the snapshot path crossed upwards where the restart rule of
 * /root/reference/align/affineGap.go:305 (quirk Q1) changed the state / all such crossings -- each of the former can cost the CIGAR
 * at most one gap open against the score, which is what the tests of megabase pairs (no oracle finishes them) check.
 * which = 5 / 6: rows per lane / snapshot spacing of the last 64-lane affine sweep (bench.py prices its design bytes with them).
 * which = 7 / 8: reads gnx_seed_candidates voted with the table in LDS / in a slab of device memory.
 * which = 9 / 10: pairs the fast path's gapless certificate certified by its N-free rule (they skipped sweep and walk) / pairs offered
 * to it.  which = 11: pairs it certified whose read holds an N (counted in the kernel).
 * which = 14: pairs that only the edge rule graded on the end diagonals certified (9 + 11 + 14 = all certified pairs; 9 and 11 keep
 * counting what the older rules admit).
 * which = 12 / 13: fast-path calls that found the plans of the previous call on the device (equal lengths) / that built and uploaded
 * their plans.
 * reset != 0 zeroes the counter after reading (3 and 4 together). */
int gnx_debug_counter(int which, int reset, int64_t *out);
/* Diagnostics: dirties the workspace.  Every device and pinned buffer of every initialised context that is SCRATCH -- written by a call
 * before that call reads it -- is filled over its whole capacity with the 32-bit `pattern`; of the buffers that hold STATE a later call may
 * read (the resident reference, the reference index, the seed index, the open pile and its logs) only the slack behind what their owner
 * wrote.  The fast path's cached plans are dropped.  A call after it must compute what it computes on a fresh workspace
 * (tests/test_scratch_state_gpu.py).  out_buffers / out_bytes (may be NULL): buffers and bytes filled.  GNX_EDEVICE if
 * a fill did not land.  Refused with GNX_EINVAL unless the process runs with GNX_DEBUG_ENTRY=1. */
int gnx_debug_fill_scratch(uint32_t pattern, int64_t *out_buffers, int64_t *out_bytes);
/* Diagnostics (tests only), host only -- no device is needed: the gapless certificate of the fast path for one
 * global AffineGap pair, a = the read (n bases), b = its window (m bases): a naive scan for exact K-mer matches, then the decision
 * arithmetic the kernel runs (K = 16 there).  out[0 .. 4) = certified (0 / 1), the diagonal c, d* (trailing read bases that sit on
 * the window's last columns), the score.  A window that holds a byte >= 5 is never certified (the kernel raises the sweep's error for
 * it).  Refused with GNX_EINVAL unless the process runs with GNX_DEBUG_ENTRY=1. */
int gnx_debug_gapless_certificate(const gnx_params *p, const uint8_t *a, int64_t n, const uint8_t *b, int64_t m, int64_t K, int64_t *out);
/* The same with reads that hold N admitted (the kernel's rule before its graded edge test; DESIGN.md 4.22, "Reads that hold N"): the 16-mers that hold an N
 * are left out of the scan, an N row counts beside the imperfect rows in the thresholds.  out[0 .. 6) = certified (0 / 1), c, d*, the
 * score, whether the edge rule decided (-o < deficit < -2o), the number of N in the read.  Same conditions as above. */
int gnx_debug_gapless_certificate_n(const gnx_params *p, const uint8_t *a, int64_t n, const uint8_t *b, int64_t m, int64_t K, int64_t *out);
/* The same with the edge rule graded by the known end diagonals, as the kernel decides ("The edge rule on the known end
 * diagonals"): the rule above, then, where it fails at the edge rule's corners only, corners bounded by the window's real bytes on its
 * first and last columns.  out[0 .. 8) = the six fields above, admitted by the graded test only (0 / 1), the largest grade j at which
 * the bounds without the bytes would have refused (-1: none, or not admitted by the graded test).  Same conditions as above. */
int gnx_debug_gapless_certificate_edge(const gnx_params *p, const uint8_t *a, int64_t n, const uint8_t *b, int64_t m, int64_t K, int64_t *out);

/* ---- "next" row N1: chunk and multiple-alignment variants (what cmd/faChunkAlign and popgen/dunn.go run) ---- */
/* align.AffineGapChunk (/root/reference/align/affineGap_highMem.go:227-268): the affine DP over chunks of chunk_size
 * bases (cell score = ungapped score of two chunks, gapExtend*chunkSize, run lengths in bases).  p->mode must be
 * GNX_AFFINE_GAP_HIGHMEM.  Lengths that are not multiples of chunk_size -> GNX_EINVAL (the Go code log.Fatalf's). */
int gnx_affine_gap_chunk_batch(const gnx_params *p, int64_t chunk_size, int64_t n_pairs,
                               const uint8_t *alpha_cat, const int64_t *alpha_off, const uint8_t *beta_cat, const int64_t *beta_off,
                               int64_t *out_score, gnx_cigar **out_ops, int64_t **out_ops_off);

/* align.multipleAffineGap (chunk_size 1, affineGap_highMem.go:270-306) and multipleAffineGapChunk (:308-353) on a batch
 * of pairs of alignment blocks ("groups"): group g holds group_nseq[g] sequences of group_len[g] bases, sequence-major,
 * at group_bases[group_off[g] ..); bases may be lower case or dna.Gap.  Pair q aligns group pair_a[q] against pair_b[q]
 * with the column score of align/multiAlign.go:82-110.  This is the inner loop of AllSeqAffine / AllSeqAffineChunk
 * (multiAlign.go:27-78): one call evaluates all x<y group pairs of a progressive-alignment round. */
int gnx_multiple_affine_gap_batch(const gnx_params *p, int64_t chunk_size, int64_t n_groups, const uint8_t *group_bases,
                                  const int64_t *group_off, const int32_t *group_nseq, const int64_t *group_len,
                                  int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                                  int64_t *out_score, gnx_cigar **out_ops, int64_t **out_ops_off);

/* Score-only twins of the two entries above (an extension: what a progressive-alignment round needs to choose its pair): the same
 * arguments minus out_ops / out_ops_off, the same validation and the same return codes for the same inputs (GNX_EINVAL for another
 * mode, lengths that are not multiples of chunk_size or bad pointers, GNX_EBASE, GNX_EDIVZERO, GNX_ERANGE only where the twin returns
 * it; GNX_EBASE and GNX_EDIVZERO are reported before any score is written; GNX_EDEVICE without a device, after the argument, mode and
 * chunk-size checks).  Contract: out_score[q] equals the score the twin returns for pair q.  One context, like the twins.
 * The score-matrix stage is the twins'.  The DP is the score sweep with explicit cell scores (gnx_timing.fast_path == 9) when
 * gapOpen <= 0, every pair has both sides non-empty, the shorter side is at most 10 240 chunk cells, (nc + mc + 2) * 2 * max|penalty|
 * is below 2^30 and every entry s - 2e and gapOpen are inside +-16 000 -- penalties and scores scaled by chunk_size, e = gapExtend *
 * chunk_size; that route allocates no CIGAR, no direction words and no traceback buffers.  Everything else (gapOpen > 0, an empty
 * side, a call the twin runs in int64, pairs beyond those bounds, GNX_SCORE_SWEEP=0) runs the route the twin takes and leaves the
 * CIGAR on the device. */
int gnx_affine_gap_chunk_score_batch(const gnx_params *p, int64_t chunk_size, int64_t n_pairs,
                                     const uint8_t *alpha_cat, const int64_t *alpha_off, const uint8_t *beta_cat, const int64_t *beta_off,
                                     int64_t *out_score);
int gnx_multiple_affine_gap_score_batch(const gnx_params *p, int64_t chunk_size, int64_t n_groups, const uint8_t *group_bases,
                                        const int64_t *group_off, const int32_t *group_nseq, const int64_t *group_len,
                                        int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b, int64_t *out_score);

/* ---- "next" row N2: the seed-extension DPs of the graph aligner (what cmd/gsw spends its DP time in) ------------------ */
/* genomeGraph.LeftDynamicAln  (/root/reference/genomeGraph/search.go:234-276): constant gap, borders 0, cell values clamped
 *   at 0; traceback from (len(alpha), len(beta)) while the cell value is > 0.  Returns m[n][m], the route and the (i, j) where
 *   the walk stopped.
 * genomeGraph.RightDynamicAln (search.go:278-321): constant gap with Needleman-Wunsch borders; the alignment ends at the first
 *   row-major cell holding the maximum (> 0) and is traced back to (0, 0).  Returns that maximum, the route and (maxI, maxJ).
 * Both use cigar.TripleMaxTrace (cigar/tools.go:58-66: M >= I >= D).  The route is in TRACEBACK order, exactly as the
 * reference builds it when it is called with an empty dynamicScore.route (callers reverse it, search.go:196,228); ops are
 * GNX_COL_M/I/D for cigar 'M'/'I'/'D', gnx_cigar has the layout of cigar.Cigar{RunLength int; Op byte} on amd64.
 * gap_pen must be <= 0 (gsw passes -600, search.go:176,210).  RIGHT packs (score, column) into one int32 per row:
 * sequences up to 4095 bases and (n+m+2)*max|penalty| < 2^19, else GNX_ERANGE (the reference's matrix is 2480 x 2480,
 * search.go:22).  One call replaces the per-seed calls of GraphSmithWatermanToGiraf (toGiraf.go:58-59) for a batch of reads. */
#define GNX_GSW_LEFT 0
#define GNX_GSW_RIGHT 1
int gnx_gsw_extend_batch(int side, const int64_t *scores, int64_t gap_pen, int64_t n_pairs,
                         const uint8_t *alpha_cat, const int64_t *alpha_off, const uint8_t *beta_cat, const int64_t *beta_off,
                         int64_t *out_score, int64_t *out_end_i, int64_t *out_end_j, gnx_cigar **out_ops, int64_t **out_ops_off);

/* The graph aligner's read path, one call per batch of reads: genomeGraph.GraphSmithWatermanToGiraf (/root/reference/genomeGraph/toGiraf.go:17-72)
 * for every read -- seeds (seedMapMemPool, search.go:549-590), seedCouldBeBetter pruning (index.go:102-121), Left / RightAlignTraversal
 * (search.go:166-232) with their DPs -- and, with paired != 0, WrapPairGiraf's flags (toGiraf.go:117-140; reads 2k / 2k+1 = the mates of pair k).
 * What the reference spreads over `-t` worker goroutines (genomeGraph/routines.go:12-65, cmd/gsw) runs here as: seed search and extension
 * DPs of the whole batch on the device, the per-read bookkeeping between them on `threads` host threads (0 = GNX_GSW_THREADS, else
 * min(hardware threads, 16)).  The graph handle keeps the nodes, the edges and the seed index (IndexGenomeIntoMap, index.go:21-59; resident on
 * the device between calls).  Results in input order: out_girafs[r] with its node ids at out_nodes[node_off ..) and its cigar
 * (cigar.Cigar{RunLength, Op}: op = the ASCII byte 'M' 'I' 'D' 'S', as cigar.Cigar.Op holds it) at out_cigars[cigar_off ..); a read on
 * which the Go code panics (getLeftTargetBases with a short Prev node, search.go:139) has panicked = 1 and nothing else.  The three
 * arrays are malloc'd: gnx_free().  Not pinned by the reference's tests (parity contract: DESIGN.md section 6). */
typedef struct gnx_gsw_graph gnx_gsw_graph;
typedef struct gnx_giraf {
    int64_t q_start, q_end, t_start, t_end, aln_score; /* giraf.Giraf: QStart, QEnd, Path.TStart, Path.TEnd, AlnScore */
    int64_t node_off, n_nodes;                         /* Path.Nodes */
    int64_t cigar_off, n_cigar;                        /* Cigar (has_cigar = 0: nil) */
    int32_t pos_strand, flag, map_q, has_cigar;
    int32_t seq_is_rc;                                 /* Seq is the read's reverse complement (1) or the read (0) */
    int32_t panicked;
} gnx_giraf;
int gnx_gsw_graph_create(const uint8_t *node_cat, const int64_t *node_off, int64_t n_nodes, const int32_t *edge_from, const int32_t *edge_to,
                         int64_t n_edges, int seed_len, int seed_step, gnx_gsw_graph **out);
void gnx_gsw_graph_free(gnx_gsw_graph *g);
int gnx_gsw_map_reads(gnx_gsw_graph *g, const uint8_t *read_cat, const int64_t *read_off, int64_t n_reads, int paired, const int64_t *scores,
                      int64_t gap_pen, int threads, gnx_giraf **out_girafs, uint32_t **out_nodes, gnx_cigar **out_cigars);

/* ---- "next" row N4: the seed index and the seed search of the graph aligner (what cmd/gsw does before its DPs) ----------------- */
/* genomeGraph.IndexGenomeIntoMap (/root/reference/genomeGraph/index.go:21-43) for the k-mers inside nodes: node k is
 * node_cat[node_off[k] .. node_off[k+1]) (dna.Base bytes, N allowed); positions 0, seed_step, ... of every node; k-mers with an N
 * are skipped.  Output = the map as two arrays sorted by key (k-mer code, index.go `dnaToNumber`), equal keys in the reference's
 * insertion order (node, position); locations are `node << 32 | pos` (ChromAndPosToNumber).  malloc'd, gnx_free().  The k-mers
 * that run across node borders (index.go:34-38) are left to the host, which merges them and calls gnx_seed_index_set.
 * A build that has k-mer positions to look at works in the buffers of the resident index: nothing is resident after it (a
 * gnx_seed_find_batch answers GNX_EINVAL until the next set), and it ends the current generation (gnx_seed_find_batch_gen: GNX_ESTALE). */
int gnx_seed_index_build(const uint8_t *node_cat, const int64_t *node_off, int64_t n_nodes, int seed_len, int seed_step,
                         uint64_t **out_keys, uint64_t **out_locs, int64_t *out_n);
/* Make an index (+ the nodes, packed like dnaTwoBit does it) resident on the device for gnx_seed_find_batch. */
int gnx_seed_index_set(const uint64_t *keys, const uint64_t *locs, int64_t n_index, const uint8_t *node_cat, const int64_t *node_off,
                       int64_t n_nodes, int seed_len);
/* The hash-lookup / exact-match part of genomeGraph.seedMapMemPool (search.go:549-590) for a batch of reads: for every read
 * position and strand (0 = read, 1 = reverse complement) every index hit, extended to the left inside its node
 * (dnaTwoBit.CountLeftMatches) and from there to the right (CountRightMatches, the first step of extendToTheRightDev).  Hits of
 * read r are out_hits[out_hit_off[r] .. out_hit_off[r+1]) in the reference's order of discovery.  A hit whose right end reaches
 * the end of its node continues into the Next nodes on the host (as does the leftward continuation over Prev edges). */
typedef struct gnx_seed_hit {
    int32_t read_start; /* the read position whose k-mer hit */
    int32_t strand;
    int32_t node, node_start; /* target of the extended seed part */
    int32_t q_start;          /* its start in the read (strand 1: in the reverse complement) */
    int32_t right;            /* its length */
} gnx_seed_hit;
int gnx_seed_find_batch(const uint8_t *read_cat, const int64_t *read_off, int64_t n_reads, gnx_seed_hit **out_hits, int64_t **out_hit_off);
/* The device holds ONE resident index; gnx_seed_index_set + gnx_seed_find_batch are two calls, so another thread's set can land between
 * them.  Callers that share the process with other users of the index (gnx_gsw_map_reads does) use this pair instead: the set returns
 * the GENERATION it installed, the search names it and is refused with GNX_ESTALE -- inside the lock that runs the search -- when the
 * resident index is no longer that one -- replaced by another set, taken by a gnx_seed_index_build, dropped by gnx_shutdown --; the
 * caller then sets again.  (The plain pair above stays for single-threaded callers.) */
int gnx_seed_index_set_gen(const uint64_t *keys, const uint64_t *locs, int64_t n_index, const uint8_t *node_cat, const int64_t *node_off,
                           int64_t n_nodes, int seed_len, uint64_t *out_generation);
int gnx_seed_find_batch_gen(uint64_t generation, const uint8_t *read_cat, const int64_t *read_off, int64_t n_reads, gnx_seed_hit **out_hits, int64_t **out_hit_off);

#ifdef __cplusplus
}
#endif
#endif /* GNX_ALIGN_H */
