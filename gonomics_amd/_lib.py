"""ctypes binding of the C ABI declared in include/gnx_align.h.

The HIP library is the product: if libgonomics_align_hip.so is missing or a GPU is absent, calls fail
loudly (GnxError / OSError).  There is no CPU fallback and nothing here ever touches oracle/.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GNX_LIB_PATH") or os.path.join(_HERE, "libgonomics_align_hip.so")

GNX_OK, GNX_EINVAL, GNX_EBASE, GNX_EEMPTY, GNX_ERANGE, GNX_EDEVICE, GNX_ENOMEM, GNX_ECAPACITY, GNX_ETRACE, GNX_EDIVZERO, GNX_ESTALE = range(11)
GNX_AFFINE_GAP, GNX_CONST_GAP, GNX_AFFINE_GAP_HIGHMEM, GNX_AFFINE_GAP_LOCAL, GNX_CONST_GAP_HIGHMEM = range(5)

EXPORTS = ["gnx_device_count", "gnx_init", "gnx_shutdown", "gnx_last_error", "gnx_free", "gnx_align_batch",
           "gnx_align_batch_windows", "gnx_align_pair", "gnx_align_batch_device", "gnx_get_timing",
           "gnx_affine_gap_chunk_batch", "gnx_multiple_affine_gap_batch", "gnx_gsw_extend_batch",
           "gnx_init_devices", "gnx_n_devices", "gnx_set_reference", "gnx_set_reference_synthetic", "gnx_align_batch_by_offset",
           "gnx_seed_index_build", "gnx_seed_index_set", "gnx_seed_find_batch", "gnx_seed_index_set_gen", "gnx_seed_find_batch_gen", "gnx_gsw_graph_create", "gnx_gsw_graph_free", "gnx_gsw_map_reads", "gnx_debug_occupy", "gnx_debug_counter", "gnx_debug_fill_scratch", "gnx_debug_gapless_certificate", "gnx_debug_gapless_certificate_n", "gnx_debug_gapless_certificate_edge", "gnx_reference_info",
           "gnx_score_batch", "gnx_score_batch_windows", "gnx_score_batch_by_offset", "gnx_score_batch_device",
           "gnx_locate_batch", "gnx_locate_batch_windows", "gnx_locate_batch_by_offset",
           "gnx_locate_span_batch", "gnx_locate_span_batch_windows", "gnx_locate_span_batch_by_offset",
           "gnx_affine_gap_chunk_score_batch", "gnx_multiple_affine_gap_score_batch",
           "gnx_best_of_by_offset", "gnx_best_of_windows", "gnx_best_pair_by_offset", "gnx_best_pair_windows",
           "gnx_reference_index_build", "gnx_reference_index_info", "gnx_reference_index_get", "gnx_seed_candidates",
           "gnx_summarize_batch", "gnx_summarize_batch_windows", "gnx_summarize_batch_by_offset",
           "gnx_md_batch", "gnx_md_batch_windows", "gnx_md_batch_by_offset", "gnx_mapq_batch",
           "gnx_pileup_open", "gnx_pileup_info", "gnx_pileup_add_by_offset", "gnx_pileup_get", "gnx_pileup_calls", "gnx_pileup_close",
           "gnx_pileup_track_alleles", "gnx_pileup_allele_info", "gnx_pileup_alleles", "gnx_pileup_indel_calls",
           "gnx_pileup_alleles_norm", "gnx_pileup_indel_calls_norm",
           "gnx_pileup_track_qualities", "gnx_pileup_qual_info", "gnx_pileup_add_by_offset_qual", "gnx_pileup_get_qual", "gnx_pileup_genotypes"]
GNX_XCOL_EQ, GNX_XCOL_X = 3, 4


class GnxCigar(ctypes.Structure):
    _fields_ = [("run_length", ctypes.c_int64), ("op", ctypes.c_uint8), ("_pad", ctypes.c_uint8 * 7)]


CIGAR_DTYPE = np.dtype({"names": ["run_length", "op"], "formats": [np.int64, np.uint8], "offsets": [0, 8], "itemsize": 16})


class GnxParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("_reserved", ctypes.c_int32), ("scores", ctypes.c_int64 * 25),
                ("gap_open", ctypes.c_int64), ("gap_extend", ctypes.c_int64),
                ("checkersize_i", ctypes.c_int64), ("checkersize_j", ctypes.c_int64)]


class GnxTiming(ctypes.Structure):
    _fields_ = [("fill_ms", ctypes.c_double), ("traceback_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("cells", ctypes.c_int64), ("n_launches", ctypes.c_int64), ("trace_bytes", ctypes.c_int64),
                ("dominant_ms", ctypes.c_double), ("dominant_launches", ctypes.c_int64), ("fast_path", ctypes.c_int32),
                ("_pad", ctypes.c_int32), ("host_ms", ctypes.c_double), ("stage0_ms", ctypes.c_double), ("fetch_ms", ctypes.c_double),
                ("transport", ctypes.c_int32), ("n_contexts", ctypes.c_int32), ("gather_ms", ctypes.c_double), ("bcast_ms", ctypes.c_double)]


class GnxSeedVoteOpts(ctypes.Structure):
    _fields_ = [("max_occ", ctypes.c_int32), ("bin", ctypes.c_int32), ("pad", ctypes.c_int32), ("max_cand", ctypes.c_int32),
                ("min_votes", ctypes.c_int32), ("_reserved", ctypes.c_int32 * 3)]


class GnxPairOpts(ctypes.Structure):
    _fields_ = [("min_insert", ctypes.c_int64), ("max_insert", ctypes.c_int64), ("unpaired_penalty", ctypes.c_int64), ("_reserved", ctypes.c_int64)]


SUMMARY_FIELDS = ("rescore", "alpha_used", "beta_used", "alpha_start", "alpha_end", "n_equal", "n_mismatch", "ins_bases", "del_bases", "gap_runs", "n_xops")


class GnxAlnSummary(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int64) for f in SUMMARY_FIELDS] + [("_reserved", ctypes.c_int64)]


SUMMARY_DTYPE = np.dtype([(f, np.int64) for f in SUMMARY_FIELDS] + [("_reserved", np.int64)])


class GnxPileCallOpts(ctypes.Structure):
    _fields_ = [("min_depth", ctypes.c_int32), ("min_alt", ctypes.c_int32), ("frac_num", ctypes.c_int32), ("frac_den", ctypes.c_int32),
                ("both_strands", ctypes.c_int32), ("_reserved", ctypes.c_int32)]


# gnx_pile: one reference position, 64 bytes; gnx_pile_call: one call, 24 bytes
PILE_DTYPE = np.dtype([("base", np.int32, (2, 5)), ("del", np.int32, (2,)), ("ins", np.int32, (2,)), ("_reserved", np.int32, (2,))])
PILE_CALL_DTYPE = np.dtype({"names": ["pos", "depth", "count", "count_fwd", "kind", "ref", "alt", "_pad"],
                            "formats": [np.int64, np.int32, np.int32, np.int32, np.uint8, np.uint8, np.uint8, np.uint8],
                            "offsets": [0, 8, 12, 16, 20, 21, 22, 23], "itemsize": 24})


# gnx_pile_allele: one distinct indel allele with its counts, 32 bytes; gnx_pile_indel_call: the allele, the depth and the reference code, 40 bytes
PILE_ALLELE_DTYPE = np.dtype({"names": ["pos", "seq", "length", "count", "count_fwd", "kind", "_pad"],
                              "formats": [np.int64, np.uint64, np.int32, np.int32, np.int32, np.uint8, (np.uint8, (3,))],
                              "offsets": [0, 8, 16, 20, 24, 28, 29], "itemsize": 32})
PILE_INDEL_CALL_DTYPE = np.dtype({"names": ["pos", "seq", "length", "count", "count_fwd", "kind", "_pad", "depth", "ref", "_pad2"],
                                  "formats": [np.int64, np.uint64, np.int32, np.int32, np.int32, np.uint8, (np.uint8, (3,)), np.int32, np.uint8, (np.uint8, (3,))],
                                  "offsets": [0, 8, 16, 20, 24, 28, 29, 32, 36, 37], "itemsize": 40})
PILE_SEQ_MAX = 21  # inserted bases whose sequence an allele keeps


class GnxGenoOpts(ctypes.Structure):
    _fields_ = [("min_depth", ctypes.c_int32), ("min_qual", ctypes.c_int32), ("prior_het", ctypes.c_int32), ("prior_hom", ctypes.c_int32),
                ("_reserved", ctypes.c_int32 * 2)]


# gnx_pile_genotype: one diploid SNP genotype, 48 bytes (centi-Phred pl / gq / qual)
PILE_GENOTYPE_DTYPE = np.dtype({"names": ["pos", "pl", "gq", "qual", "depth", "ref_count", "alt_count", "alt_fwd", "gt", "ref", "alt", "_pad"],
                                "formats": [np.int64, (np.int32, (3,)), np.int32, np.int32, np.int32, np.int32, np.int32, np.int32, np.uint8, np.uint8, np.uint8, np.uint8],
                                "offsets": [0, 8, 20, 24, 28, 32, 36, 40, 44, 45, 46, 47], "itemsize": 48})
QUAL_MAX = 93                      # a quality byte above it counts as 93
QUAL_MAX_READS = (2 ** 31 - 1) // 93  # reads a quality pile takes: 23 091 222


class GnxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gnx error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load the HIP library (once).  Raises OSError if it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        c_p = ctypes.c_void_p
        i64 = ctypes.c_int64
        L.gnx_device_count.restype = ctypes.c_int
        L.gnx_init.argtypes = [ctypes.c_int, i64]
        L.gnx_init.restype = ctypes.c_int
        L.gnx_shutdown.restype = None
        L.gnx_last_error.restype = ctypes.c_char_p
        L.gnx_free.argtypes = [c_p]
        L.gnx_free.restype = None
        L.gnx_align_batch.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p,
                                      ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_align_batch.restype = ctypes.c_int
        L.gnx_align_batch_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p,
                                              ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_align_batch_windows.restype = ctypes.c_int
        L.gnx_align_pair.argtypes = [ctypes.POINTER(GnxParams), c_p, i64, c_p, i64, ctypes.POINTER(i64),
                                     ctypes.POINTER(c_p), ctypes.POINTER(i64)]
        L.gnx_align_pair.restype = ctypes.c_int
        L.gnx_align_batch_device.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                             c_p, c_p, i64, c_p, ctypes.POINTER(i64), c_p]
        L.gnx_align_batch_device.restype = ctypes.c_int
        L.gnx_affine_gap_chunk_batch.argtypes = [ctypes.POINTER(GnxParams), i64, i64, c_p, c_p, c_p, c_p, c_p,
                                                 ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_affine_gap_chunk_batch.restype = ctypes.c_int
        L.gnx_multiple_affine_gap_batch.argtypes = [ctypes.POINTER(GnxParams), i64, i64, c_p, c_p, c_p, c_p, i64, c_p, c_p, c_p,
                                                    ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_multiple_affine_gap_batch.restype = ctypes.c_int
        if hasattr(L, "gnx_affine_gap_chunk_score_batch"):  # (absent from older builds loaded through GNX_LIB_PATH for A/B runs)
            L.gnx_affine_gap_chunk_score_batch.argtypes = [ctypes.POINTER(GnxParams), i64, i64, c_p, c_p, c_p, c_p, c_p]
            L.gnx_affine_gap_chunk_score_batch.restype = ctypes.c_int
            L.gnx_multiple_affine_gap_score_batch.argtypes = [ctypes.POINTER(GnxParams), i64, i64, c_p, c_p, c_p, c_p, i64, c_p, c_p, c_p]
            L.gnx_multiple_affine_gap_score_batch.restype = ctypes.c_int
        L.gnx_gsw_extend_batch.argtypes = [ctypes.c_int, c_p, i64, i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                           ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_gsw_extend_batch.restype = ctypes.c_int
        L.gnx_init_devices.argtypes = [ctypes.c_int, c_p, i64]
        L.gnx_init_devices.restype = ctypes.c_int
        L.gnx_n_devices.restype = ctypes.c_int
        L.gnx_set_reference.argtypes = [c_p, i64]
        L.gnx_set_reference.restype = ctypes.c_int
        L.gnx_set_reference_synthetic.argtypes = [i64, ctypes.c_uint64]
        L.gnx_set_reference_synthetic.restype = ctypes.c_int
        L.gnx_align_batch_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_align_batch_by_offset.restype = ctypes.c_int
        L.gnx_score_batch.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p]
        L.gnx_score_batch.restype = ctypes.c_int
        L.gnx_score_batch_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p]
        L.gnx_score_batch_windows.restype = ctypes.c_int
        L.gnx_score_batch_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p]
        L.gnx_score_batch_by_offset.restype = ctypes.c_int
        L.gnx_score_batch_device.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
        L.gnx_score_batch_device.restype = ctypes.c_int
        L.gnx_locate_batch.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p]
        L.gnx_locate_batch.restype = ctypes.c_int
        L.gnx_locate_batch_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p]
        L.gnx_locate_batch_windows.restype = ctypes.c_int
        L.gnx_locate_batch_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p]
        L.gnx_locate_batch_by_offset.restype = ctypes.c_int
        L.gnx_locate_span_batch.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
        L.gnx_locate_span_batch.restype = ctypes.c_int
        L.gnx_locate_span_batch_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p]
        L.gnx_locate_span_batch_windows.restype = ctypes.c_int
        L.gnx_locate_span_batch_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
        L.gnx_locate_span_batch_by_offset.restype = ctypes.c_int
        L.gnx_best_of_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_best_of_by_offset.restype = ctypes.c_int
        L.gnx_best_of_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_best_of_windows.restype = ctypes.c_int
        L.gnx_best_pair_by_offset.argtypes = [ctypes.POINTER(GnxParams), ctypes.POINTER(GnxPairOpts), i64, c_p, c_p] + [c_p] * 14 + [ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_best_pair_by_offset.restype = ctypes.c_int
        L.gnx_best_pair_windows.argtypes = [ctypes.POINTER(GnxParams), ctypes.POINTER(GnxPairOpts), i64, c_p, c_p, c_p, i64] + [c_p] * 14 + [ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_best_pair_windows.restype = ctypes.c_int
        L.gnx_reference_index_build.argtypes = [ctypes.c_int, ctypes.c_int]
        L.gnx_reference_index_build.restype = ctypes.c_int
        L.gnx_reference_index_info.argtypes = [ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.gnx_reference_index_info.restype = ctypes.c_int
        L.gnx_reference_index_get.argtypes = [ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(i64)]
        L.gnx_reference_index_get.restype = ctypes.c_int
        L.gnx_seed_candidates.argtypes = [ctypes.POINTER(GnxSeedVoteOpts), i64, c_p, c_p] + [ctypes.POINTER(c_p)] * 5
        L.gnx_seed_candidates.restype = ctypes.c_int
        if hasattr(L, "gnx_summarize_batch"):  # (absent from older builds loaded through GNX_LIB_PATH for A/B runs)
            L.gnx_summarize_batch.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_summarize_batch.restype = ctypes.c_int
            L.gnx_summarize_batch_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_summarize_batch_windows.restype = ctypes.c_int
            L.gnx_summarize_batch_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_summarize_batch_by_offset.restype = ctypes.c_int
        if hasattr(L, "gnx_md_batch"):
            L.gnx_md_batch.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_md_batch.restype = ctypes.c_int
            L.gnx_md_batch_windows.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, i64, c_p, c_p, c_p, i64, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_md_batch_windows.restype = ctypes.c_int
            L.gnx_md_batch_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_md_batch_by_offset.restype = ctypes.c_int
            L.gnx_mapq_batch.argtypes = [i64, c_p, c_p, c_p]
            L.gnx_mapq_batch.restype = ctypes.c_int
        if hasattr(L, "gnx_pileup_open"):
            L.gnx_pileup_open.argtypes = [i64, i64]
            L.gnx_pileup_open.restype = ctypes.c_int
            L.gnx_pileup_info.argtypes = [c_p, c_p, c_p, c_p]
            L.gnx_pileup_info.restype = ctypes.c_int
            L.gnx_pileup_add_by_offset.argtypes = [ctypes.POINTER(GnxParams), i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
            L.gnx_pileup_add_by_offset.restype = ctypes.c_int
            L.gnx_pileup_get.argtypes = [i64, i64, c_p]
            L.gnx_pileup_get.restype = ctypes.c_int
            L.gnx_pileup_calls.argtypes = [ctypes.POINTER(GnxPileCallOpts), ctypes.POINTER(c_p), ctypes.POINTER(i64)]
            L.gnx_pileup_calls.restype = ctypes.c_int
            L.gnx_pileup_close.argtypes = []
            L.gnx_pileup_close.restype = ctypes.c_int
        if hasattr(L, "gnx_pileup_track_alleles"):
            L.gnx_pileup_track_alleles.argtypes = [i64]
            L.gnx_pileup_track_alleles.restype = ctypes.c_int
            L.gnx_pileup_allele_info.argtypes = [c_p, c_p, c_p]
            L.gnx_pileup_allele_info.restype = ctypes.c_int
            L.gnx_pileup_alleles.argtypes = [ctypes.POINTER(c_p), ctypes.POINTER(i64)]
            L.gnx_pileup_alleles.restype = ctypes.c_int
            L.gnx_pileup_indel_calls.argtypes = [ctypes.POINTER(GnxPileCallOpts), ctypes.POINTER(c_p), ctypes.POINTER(i64)]
            L.gnx_pileup_indel_calls.restype = ctypes.c_int
        if hasattr(L, "gnx_pileup_alleles_norm"):
            L.gnx_pileup_alleles_norm.argtypes = L.gnx_pileup_alleles.argtypes
            L.gnx_pileup_alleles_norm.restype = ctypes.c_int
            L.gnx_pileup_indel_calls_norm.argtypes = L.gnx_pileup_indel_calls.argtypes
            L.gnx_pileup_indel_calls_norm.restype = ctypes.c_int
        if hasattr(L, "gnx_pileup_track_qualities"):
            L.gnx_pileup_track_qualities.argtypes = [ctypes.c_int32]
            L.gnx_pileup_track_qualities.restype = ctypes.c_int
            L.gnx_pileup_qual_info.argtypes = [c_p, c_p, c_p]
            L.gnx_pileup_qual_info.restype = ctypes.c_int
            L.gnx_pileup_add_by_offset_qual.argtypes = L.gnx_pileup_add_by_offset.argtypes + [c_p]
            L.gnx_pileup_add_by_offset_qual.restype = ctypes.c_int
            L.gnx_pileup_get_qual.argtypes = [i64, i64, c_p]
            L.gnx_pileup_get_qual.restype = ctypes.c_int
            L.gnx_pileup_genotypes.argtypes = [ctypes.POINTER(GnxGenoOpts), ctypes.POINTER(c_p), ctypes.POINTER(i64)]
            L.gnx_pileup_genotypes.restype = ctypes.c_int
        L.gnx_seed_index_build.argtypes = [c_p, c_p, i64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(i64)]
        L.gnx_seed_index_build.restype = ctypes.c_int
        L.gnx_seed_index_set.argtypes = [c_p, c_p, i64, c_p, c_p, i64, ctypes.c_int]
        L.gnx_seed_index_set.restype = ctypes.c_int
        L.gnx_seed_find_batch.argtypes = [c_p, c_p, i64, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_seed_find_batch.restype = ctypes.c_int
        L.gnx_seed_index_set_gen.argtypes = [c_p, c_p, i64, c_p, c_p, i64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        L.gnx_seed_index_set_gen.restype = ctypes.c_int
        L.gnx_seed_find_batch_gen.argtypes = [ctypes.c_uint64, c_p, c_p, i64, ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
        L.gnx_seed_find_batch_gen.restype = ctypes.c_int
        if hasattr(L, "gnx_gsw_map_reads"):
            L.gnx_gsw_graph_create.argtypes = [c_p, c_p, i64, c_p, c_p, i64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_p)]
            L.gnx_gsw_graph_create.restype = ctypes.c_int
            L.gnx_gsw_graph_free.argtypes = [c_p]
            L.gnx_gsw_graph_free.restype = None
            L.gnx_gsw_map_reads.argtypes = [c_p, c_p, c_p, i64, ctypes.c_int, c_p, i64, ctypes.c_int, ctypes.POINTER(c_p), ctypes.POINTER(c_p), ctypes.POINTER(c_p)]
            L.gnx_gsw_map_reads.restype = ctypes.c_int
        L.gnx_get_timing.argtypes = [ctypes.POINTER(GnxTiming)]
        L.gnx_get_timing.restype = ctypes.c_int
        if hasattr(L, "gnx_debug_occupy"):  # (absent from older builds loaded through GNX_LIB_PATH for A/B runs)
            L.gnx_debug_occupy.argtypes = [ctypes.c_int, ctypes.c_int]
            L.gnx_debug_occupy.restype = ctypes.c_int
        if hasattr(L, "gnx_debug_counter"):
            L.gnx_debug_counter.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
            L.gnx_debug_counter.restype = ctypes.c_int
        if hasattr(L, "gnx_debug_gapless_certificate"):
            L.gnx_debug_gapless_certificate.argtypes = [ctypes.POINTER(GnxParams), c_p, i64, c_p, i64, i64, c_p]
            L.gnx_debug_gapless_certificate.restype = ctypes.c_int
        if hasattr(L, "gnx_debug_gapless_certificate_n"):
            L.gnx_debug_gapless_certificate_n.argtypes = [ctypes.POINTER(GnxParams), c_p, i64, c_p, i64, i64, c_p]
            L.gnx_debug_gapless_certificate_n.restype = ctypes.c_int
        if hasattr(L, "gnx_debug_gapless_certificate_edge"):
            L.gnx_debug_gapless_certificate_edge.argtypes = [ctypes.POINTER(GnxParams), c_p, i64, c_p, i64, i64, c_p]
            L.gnx_debug_gapless_certificate_edge.restype = ctypes.c_int
        if hasattr(L, "gnx_debug_fill_scratch"):
            L.gnx_debug_fill_scratch.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
            L.gnx_debug_fill_scratch.restype = ctypes.c_int
        _lib = L
    return _lib


def debug_counter(which=0, reset=True):
    v = ctypes.c_int64()
    check(lib().gnx_debug_counter(which, 1 if reset else 0, ctypes.byref(v)))
    return int(v.value)


def debug_fill_scratch(pattern):
    """Dirties the workspace of every initialised context with a 32-bit pattern (needs GNX_DEBUG_ENTRY=1): scratch buffers over their whole
    capacity, state buffers behind what their owner wrote; the fast path's cached plans are dropped.  Returns (buffers, bytes) filled."""
    nb, by = ctypes.c_int64(), ctypes.c_int64()
    check(lib().gnx_debug_fill_scratch(ctypes.c_uint32(int(pattern) & 0xFFFFFFFF), ctypes.byref(nb), ctypes.byref(by)))
    return int(nb.value), int(by.value)


def debug_gapless_certificate(params, a, b, K=16):
    """The fast path's gapless certificate for one pair, on the host (needs GNX_DEBUG_ENTRY=1): (certified, c, d_star, score)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    out = np.zeros(4, dtype=np.int64)
    check(lib().gnx_debug_gapless_certificate(ctypes.byref(params), a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], int(K), out.ctypes.data))
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3])


def debug_gapless_certificate_n(params, a, b, K=16):
    """The same with reads that hold N admitted, the kernel's rule before its graded edge test: (certified, c, d_star, score, edge rule decided, N in the read)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    out = np.zeros(6, dtype=np.int64)
    check(lib().gnx_debug_gapless_certificate_n(ctypes.byref(params), a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], int(K), out.ctypes.data))
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3]), bool(out[4]), int(out[5])


def debug_gapless_certificate_edge(params, a, b, K=16):
    """The same with the edge rule graded by the window's first and last columns, as the kernel decides: the six fields above, admitted by
    the graded test only, the largest grade at which the bounds without the bytes would have refused (-1: none)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    out = np.zeros(8, dtype=np.int64)
    check(lib().gnx_debug_gapless_certificate_edge(ctypes.byref(params), a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0], int(K), out.ctypes.data))
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3]), bool(out[4]), int(out[5]), bool(out[6]), int(out[7])


def check(rc):
    if rc != GNX_OK:
        raise GnxError(rc, lib().gnx_last_error().decode("utf-8", "replace"))


def make_params(mode, scores, gap_open, gap_extend=0, checkersize_i=10000, checkersize_j=10000):
    p = GnxParams()
    p.mode = mode
    flat = [int(v) for row in scores for v in row]
    if len(flat) != 25:
        raise ValueError("scores must be a 5x5 matrix")
    for k, v in enumerate(flat):
        p.scores[k] = v
    p.gap_open = int(gap_open)
    p.gap_extend = int(gap_extend)
    p.checkersize_i = int(checkersize_i)
    p.checkersize_j = int(checkersize_j)
    return p


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _take(ops_p, off_p, n_pairs):
    L = lib()
    off = np.ctypeslib.as_array(ctypes.cast(off_p, ctypes.POINTER(ctypes.c_int64)), shape=(n_pairs + 1,)).copy()
    total = int(off[-1])
    if total:
        buf = (ctypes.c_char * (total * 16)).from_address(ops_p.value)
        ops = np.frombuffer(buf, dtype=CIGAR_DTYPE, count=total).copy()
    else:
        ops = np.zeros(0, dtype=CIGAR_DTYPE)
    L.gnx_free(ops_p)
    L.gnx_free(off_p)
    return ops, off


def align_batch_windows(params, a_buf, a_start, a_len, b_buf, b_start, b_len):
    """Host-buffer batch over windows of shared buffers.  Returns (scores[int64], ops[CIGAR_DTYPE], off[int64])."""
    L = lib()
    a_buf, b_buf = _u8(a_buf), _u8(b_buf)
    a_start, a_len, b_start, b_len = _i64(a_start), _i64(a_len), _i64(b_start), _i64(b_len)
    n = int(a_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_align_batch_windows(ctypes.byref(params), n, a_buf.ctypes.data, a_buf.shape[0], a_start.ctypes.data, a_len.ctypes.data,
                                    b_buf.ctypes.data, b_buf.shape[0], b_start.ctypes.data, b_len.ctypes.data,
                                    scores.ctypes.data, ctypes.byref(ops_p), ctypes.byref(off_p)))
    ops, off = _take(ops_p, off_p, n)
    return scores[:n], ops, off


class RawResult:
    """Results of a host-buffer call as the C ABI hands them over: `scores` is the caller's array, `ops` / `off` are VIEWS of the
    pinned arrays the library returned (no copy -- what a cgo shim wraps with unsafe.Slice); free() gives them back (gnx_free)."""

    def __init__(self, scores, ops_p, off_p, n):
        self.scores, self._ops_p, self._off_p, self.n = scores, ops_p, off_p, n
        self.off = np.ctypeslib.as_array(ctypes.cast(off_p, ctypes.POINTER(ctypes.c_int64)), shape=(n + 1,))
        total = int(self.off[-1])
        if total:
            buf = (ctypes.c_char * (total * 16)).from_address(ops_p.value)
            self.ops = np.frombuffer(buf, dtype=CIGAR_DTYPE, count=total)
        else:
            self.ops = np.zeros(0, dtype=CIGAR_DTYPE)

    def copy(self):
        return self.scores[:self.n].copy(), self.ops.copy(), self.off.copy()

    def free(self):
        if self._ops_p is not None:
            L = lib()
            self.ops = self.off = None
            L.gnx_free(self._ops_p)
            L.gnx_free(self._off_p)
            self._ops_p = self._off_p = None


def align_batch_windows_raw(params, a_buf, a_start, a_len, b_buf, b_start, b_len, scores=None):
    """gnx_align_batch_windows without the binding's extra copy of the results (arguments must already be contiguous uint8 / int64
    arrays).  Returns a RawResult; call .free() when done."""
    L = lib()
    n = int(a_start.shape[0])
    if scores is None:
        scores = np.zeros(max(n, 1), dtype=np.int64)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_align_batch_windows(ctypes.byref(params), n, a_buf.ctypes.data, a_buf.shape[0], a_start.ctypes.data, a_len.ctypes.data,
                                    b_buf.ctypes.data, b_buf.shape[0], b_start.ctypes.data, b_len.ctypes.data,
                                    scores.ctypes.data, ctypes.byref(ops_p), ctypes.byref(off_p)))
    return RawResult(scores, ops_p, off_p, n)


def init_devices(devices=None, workspace_bytes=0):
    """One context per listed device in this process (gnx_init_devices); devices=None: every visible GPU."""
    L = lib()
    if devices is None:
        check(L.gnx_init_devices(0, None, int(workspace_bytes)))
    else:
        d = np.ascontiguousarray(devices, dtype=np.int32)
        check(L.gnx_init_devices(int(d.shape[0]), d.ctypes.data, int(workspace_bytes)))
    return L.gnx_n_devices()


def set_reference(ref):
    ref = _u8(ref)
    check(lib().gnx_set_reference(ref.ctypes.data, ref.shape[0]))


def reference_info():
    """(bases, device bytes per context, 64-base blocks on the exception list) of the resident, packed reference"""
    L = lib()
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    L.gnx_reference_info.argtypes = [ctypes.POINTER(ctypes.c_int64)] * 3
    L.gnx_reference_info.restype = ctypes.c_int
    check(L.gnx_reference_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def synthetic_reference_bases(start, length, seed):
    """Host restatement of gnx_set_reference_synthetic for bases [start, start + length) (tests and benchmarks build their oracle
    inputs from it)."""
    return synthetic_reference_positions(np.arange(start, start + length, dtype=np.int64), seed)


def synthetic_reference_positions(pos, seed):
    """... for arbitrary positions"""
    pos = np.asarray(pos).astype(np.uint64)
    w = pos >> np.uint64(5)
    with np.errstate(over="ignore"):
        x = (np.uint64(seed) ^ w) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    b = ((x >> (np.uint64(2) * (pos & np.uint64(31)))) & np.uint64(3)).astype(np.uint8)
    p = pos.astype(np.int64)
    b[(p % 50000000 < 1000) & (p >= 50000000)] = 4
    return b


def align_batch_by_offset(params, a_cat, a_off, ref_start, ref_len):
    """Reads (concatenated, a_off[n+1]) against windows of the resident reference.  Returns (scores, ops, off)."""
    L = lib()
    a_cat, a_off, ref_start, ref_len = _u8(a_cat), _i64(a_off), _i64(ref_start), _i64(ref_len)
    n = int(ref_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_align_batch_by_offset(ctypes.byref(params), n, a_cat.ctypes.data, a_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                      scores.ctypes.data, ctypes.byref(ops_p), ctypes.byref(off_p)))
    ops, off = _take(ops_p, off_p, n)
    return scores[:n], ops, off


def align_batch(params, alphas, betas):
    """Batch of independent pairs given as lists of uint8 arrays (concatenated form of the C ABI)."""
    L = lib()
    n = len(alphas)
    a_off = np.zeros(n + 1, dtype=np.int64)
    b_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        a_off[1:] = np.cumsum([len(a) for a in alphas])
        b_off[1:] = np.cumsum([len(b) for b in betas])
    a_cat = _u8(np.concatenate([_u8(a) for a in alphas])) if n and a_off[-1] else np.zeros(1, dtype=np.uint8)
    b_cat = _u8(np.concatenate([_u8(b) for b in betas])) if n and b_off[-1] else np.zeros(1, dtype=np.uint8)
    scores = np.zeros(max(n, 1), dtype=np.int64)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_align_batch(ctypes.byref(params), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data, b_off.ctypes.data,
                            scores.ctypes.data, ctypes.byref(ops_p), ctypes.byref(off_p)))
    ops, off = _take(ops_p, off_p, n)
    return scores[:n], ops, off


def _h_lens(n, h_len):
    """a host length table of the device entries as (array kept alive, pointer): None stays NULL"""
    if h_len is None:
        return None, None
    h = _i64(h_len)
    if h.shape[0] < n:
        raise ValueError("length table shorter than n_pairs")
    return h, h.ctypes.data


def align_batch_device(params, n_pairs, d_alpha_buf, d_alpha_start, d_beta_buf, d_beta_start, h_alpha_len, h_beta_len,
                       d_score, d_ops, ops_capacity, d_ops_off, stream=0, d_alpha_len=0, d_beta_len=0, want_total=True):
    """gnx_align_batch_device as the C ABI has it: every d_* is a raw device address (an int; 0 = NULL), h_*_len are host int64 arrays
    (None = NULL), stream is a hipStream_t handle as an int (0 = the NULL stream).  Returns (rc, total_ops) and never raises
    on a return code -- GNX_ECAPACITY comes back with the number of runs the whole batch needs.  want_total=False passes out_total_ops = NULL
    (total_ops is then None)."""
    keep_a, pa = _h_lens(int(n_pairs), h_alpha_len)
    keep_b, pb = _h_lens(int(n_pairs), h_beta_len)
    total = ctypes.c_int64(-1)
    rc = lib().gnx_align_batch_device(ctypes.byref(params), int(n_pairs), d_alpha_buf or None, d_alpha_start or None, d_alpha_len or None,
                                      d_beta_buf or None, d_beta_start or None, d_beta_len or None, pa, pb,
                                      d_score or None, d_ops or None, int(ops_capacity), d_ops_off or None,
                                      ctypes.byref(total) if want_total else None, stream or None)
    del keep_a, keep_b
    return int(rc), (int(total.value) if want_total else None)


def score_batch_device(params, n_pairs, d_alpha_buf, d_alpha_start, d_beta_buf, d_beta_start, h_alpha_len, h_beta_len,
                       d_score, stream=0, d_alpha_len=0, d_beta_len=0):
    """gnx_score_batch_device on raw device addresses (see align_batch_device).  Returns rc."""
    keep_a, pa = _h_lens(int(n_pairs), h_alpha_len)
    keep_b, pb = _h_lens(int(n_pairs), h_beta_len)
    rc = lib().gnx_score_batch_device(ctypes.byref(params), int(n_pairs), d_alpha_buf or None, d_alpha_start or None, d_alpha_len or None,
                                      d_beta_buf or None, d_beta_start or None, d_beta_len or None, pa, pb, d_score or None, stream or None)
    del keep_a, keep_b
    return int(rc)


def last_error():
    return lib().gnx_last_error().decode("utf-8", "replace")


def score_batch_windows(params, a_buf, a_start, a_len, b_buf, b_start, b_len):
    """gnx_score_batch_windows: the scores of align_batch_windows without the CIGARs.  Returns scores[int64]."""
    L = lib()
    a_buf, b_buf = _u8(a_buf), _u8(b_buf)
    a_start, a_len, b_start, b_len = _i64(a_start), _i64(a_len), _i64(b_start), _i64(b_len)
    n = int(a_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_score_batch_windows(ctypes.byref(params), n, a_buf.ctypes.data, a_buf.shape[0], a_start.ctypes.data, a_len.ctypes.data,
                                    b_buf.ctypes.data, b_buf.shape[0], b_start.ctypes.data, b_len.ctypes.data, scores.ctypes.data))
    return scores[:n]


def score_batch_by_offset(params, a_cat, a_off, ref_start, ref_len):
    """gnx_score_batch_by_offset: reads against windows of the resident reference, scores only."""
    L = lib()
    a_cat, a_off, ref_start, ref_len = _u8(a_cat), _i64(a_off), _i64(ref_start), _i64(ref_len)
    n = int(ref_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_score_batch_by_offset(ctypes.byref(params), n, a_cat.ctypes.data, a_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                      scores.ctypes.data))
    return scores[:n]


def score_batch(params, alphas, betas):
    """gnx_score_batch on lists of uint8 arrays.  Returns scores[int64]."""
    L = lib()
    n = len(alphas)
    a_off = np.zeros(n + 1, dtype=np.int64)
    b_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        a_off[1:] = np.cumsum([len(a) for a in alphas])
        b_off[1:] = np.cumsum([len(b) for b in betas])
    a_cat = _u8(np.concatenate([_u8(a) for a in alphas])) if n and a_off[-1] else np.zeros(1, dtype=np.uint8)
    b_cat = _u8(np.concatenate([_u8(b) for b in betas])) if n and b_off[-1] else np.zeros(1, dtype=np.uint8)
    scores = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_score_batch(ctypes.byref(params), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data, b_off.ctypes.data, scores.ctypes.data))
    return scores[:n]


# ---- locate calls (gnx_locate_*): AffineGapLocal's score and the target end of its alignment, named by role ----
def locate_batch_windows(params, t_buf, t_start, t_len, q_buf, q_start, q_len):
    """gnx_locate_batch_windows: targets and queries as windows of shared buffers.  Returns (scores[int64], target_ends[int64])."""
    L = lib()
    t_buf, q_buf = _u8(t_buf), _u8(q_buf)
    t_start, t_len, q_start, q_len = _i64(t_start), _i64(t_len), _i64(q_start), _i64(q_len)
    n = int(t_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    ends = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_locate_batch_windows(ctypes.byref(params), n, t_buf.ctypes.data, t_buf.shape[0], t_start.ctypes.data, t_len.ctypes.data,
                                     q_buf.ctypes.data, q_buf.shape[0], q_start.ctypes.data, q_len.ctypes.data, scores.ctypes.data, ends.ctypes.data))
    return scores[:n], ends[:n]


def locate_batch_by_offset(params, q_cat, q_off, ref_start, ref_len):
    """gnx_locate_batch_by_offset: reads (the queries) against windows of the resident reference (the targets)."""
    L = lib()
    q_cat, q_off, ref_start, ref_len = _u8(q_cat), _i64(q_off), _i64(ref_start), _i64(ref_len)
    n = int(ref_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    ends = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_locate_batch_by_offset(ctypes.byref(params), n, q_cat.ctypes.data, q_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                       scores.ctypes.data, ends.ctypes.data))
    return scores[:n], ends[:n]


def locate_batch(params, targets, queries):
    """gnx_locate_batch on lists of uint8 arrays.  Returns (scores[int64], target_ends[int64])."""
    L = lib()
    n = len(targets)
    t_off = np.zeros(n + 1, dtype=np.int64)
    q_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        t_off[1:] = np.cumsum([len(t) for t in targets])
        q_off[1:] = np.cumsum([len(q) for q in queries])
    t_cat = _u8(np.concatenate([_u8(t) for t in targets])) if n and t_off[-1] else np.zeros(1, dtype=np.uint8)
    q_cat = _u8(np.concatenate([_u8(q) for q in queries])) if n and q_off[-1] else np.zeros(1, dtype=np.uint8)
    scores = np.zeros(max(n, 1), dtype=np.int64)
    ends = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_locate_batch(ctypes.byref(params), n, t_cat.ctypes.data, t_off.ctypes.data, q_cat.ctypes.data, q_off.ctypes.data, scores.ctypes.data, ends.ctypes.data))
    return scores[:n], ends[:n]


# ---- span calls (gnx_locate_span_*): the locate calls plus the target start of the alignment ----
def locate_span_batch_windows(params, t_buf, t_start, t_len, q_buf, q_start, q_len):
    """gnx_locate_span_batch_windows.  Returns (scores[int64], target_starts[int64], target_ends[int64])."""
    L = lib()
    t_buf, q_buf = _u8(t_buf), _u8(q_buf)
    t_start, t_len, q_start, q_len = _i64(t_start), _i64(t_len), _i64(q_start), _i64(q_len)
    n = int(t_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    starts = np.zeros(max(n, 1), dtype=np.int64)
    ends = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_locate_span_batch_windows(ctypes.byref(params), n, t_buf.ctypes.data, t_buf.shape[0], t_start.ctypes.data, t_len.ctypes.data,
                                          q_buf.ctypes.data, q_buf.shape[0], q_start.ctypes.data, q_len.ctypes.data,
                                          scores.ctypes.data, starts.ctypes.data, ends.ctypes.data))
    return scores[:n], starts[:n], ends[:n]


def locate_span_batch_by_offset(params, q_cat, q_off, ref_start, ref_len):
    """gnx_locate_span_batch_by_offset: reads (the queries) against windows of the resident reference (the targets); positions are
    relative to each window."""
    L = lib()
    q_cat, q_off, ref_start, ref_len = _u8(q_cat), _i64(q_off), _i64(ref_start), _i64(ref_len)
    n = int(ref_start.shape[0])
    scores = np.zeros(max(n, 1), dtype=np.int64)
    starts = np.zeros(max(n, 1), dtype=np.int64)
    ends = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_locate_span_batch_by_offset(ctypes.byref(params), n, q_cat.ctypes.data, q_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                            scores.ctypes.data, starts.ctypes.data, ends.ctypes.data))
    return scores[:n], starts[:n], ends[:n]


def locate_span_batch(params, targets, queries):
    """gnx_locate_span_batch on lists of uint8 arrays.  Returns (scores[int64], target_starts[int64], target_ends[int64])."""
    L = lib()
    n = len(targets)
    t_off = np.zeros(n + 1, dtype=np.int64)
    q_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        t_off[1:] = np.cumsum([len(t) for t in targets])
        q_off[1:] = np.cumsum([len(q) for q in queries])
    t_cat = _u8(np.concatenate([_u8(t) for t in targets])) if n and t_off[-1] else np.zeros(1, dtype=np.uint8)
    q_cat = _u8(np.concatenate([_u8(q) for q in queries])) if n and q_off[-1] else np.zeros(1, dtype=np.uint8)
    scores = np.zeros(max(n, 1), dtype=np.int64)
    starts = np.zeros(max(n, 1), dtype=np.int64)
    ends = np.zeros(max(n, 1), dtype=np.int64)
    check(L.gnx_locate_span_batch(ctypes.byref(params), n, t_cat.ctypes.data, t_off.ctypes.data, q_cat.ctypes.data, q_off.ctypes.data,
                                  scores.ctypes.data, starts.ctypes.data, ends.ctypes.data))
    return scores[:n], starts[:n], ends[:n]


# ---- best of K on both strands (gnx_best_of_*): score every candidate, keep the first maximum, align the winners ----
def _best_of(params, read_cat, read_off, target, cand_off, cand_start, cand_len, cand_strand, cigar, target_end):
    L = lib()
    read_cat, read_off, cand_off = _u8(read_cat), _i64(read_off), _i64(cand_off)
    cand_start, cand_len, cand_strand = _i64(cand_start), _i64(cand_len), _u8(cand_strand)
    n, nc = int(read_off.shape[0]) - 1, int(cand_start.shape[0])
    best = np.zeros(max(n, 1), dtype=np.int32)
    scores, ends, cand = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(nc, 1), dtype=np.int64)
    if target_end is None:
        target_end = params.mode == GNX_AFFINE_GAP_LOCAL
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    tail = [cand_off.ctypes.data, cand_start.ctypes.data, cand_len.ctypes.data, cand_strand.ctypes.data, best.ctypes.data, scores.ctypes.data,
            ends.ctypes.data if target_end else None, cand.ctypes.data, ctypes.byref(ops_p) if cigar else None, ctypes.byref(off_p) if cigar else None]
    if target is None:
        check(L.gnx_best_of_by_offset(ctypes.byref(params), n, read_cat.ctypes.data, read_off.ctypes.data, *tail))
    else:
        target = _u8(target)
        check(L.gnx_best_of_windows(ctypes.byref(params), n, read_cat.ctypes.data, read_off.ctypes.data, target.ctypes.data, target.shape[0], *tail))
    ops, off = _take(ops_p, off_p, n) if cigar else (None, None)
    return best[:n], scores[:n], (ends[:n] if target_end else None), cand[:nc], ops, off


def best_of_by_offset(params, read_cat, read_off, cand_off, cand_start, cand_len, cand_strand, cigar=True, target_end=None):
    """gnx_best_of_by_offset: reads against candidate windows (cand_start, cand_len, cand_strand) of the resident reference, candidates
    of read r at cand_off[r] .. cand_off[r + 1].  Returns (best[int32], scores, target_ends or None, cand_scores, ops or None, off or
    None); target_end=None asks for the ends exactly in GNX_AFFINE_GAP_LOCAL."""
    return _best_of(params, read_cat, read_off, None, cand_off, cand_start, cand_len, cand_strand, cigar, target_end)


def best_of_windows(params, read_cat, read_off, target_buf, cand_off, cand_start, cand_len, cand_strand, cigar=True, target_end=None):
    """gnx_best_of_windows: the same with the windows taken from target_buf."""
    return _best_of(params, read_cat, read_off, target_buf, cand_off, cand_start, cand_len, cand_strand, cigar, target_end)


# ---- best proper pair (gnx_best_pair_*): best-of for mate pairs, reads 2k and 2k + 1 placed together ----
def pair_opts(min_insert, max_insert, unpaired_penalty=0):
    o = GnxPairOpts()
    o.min_insert, o.max_insert, o.unpaired_penalty = int(min_insert), int(max_insert), int(unpaired_penalty)
    return o


def _best_pair(params, opts, read_cat, read_off, target, cand_off, cand_start, cand_len, cand_strand, cigar):
    L = lib()
    read_cat, read_off, cand_off = _u8(read_cat), _i64(read_off), _i64(cand_off)
    cand_start, cand_len, cand_strand = _i64(cand_start), _i64(cand_len), _u8(cand_strand)
    n, nc = int(read_off.shape[0]) - 1, int(cand_start.shape[0])
    best = np.zeros(max(n, 1), dtype=np.int32)
    per_read = [np.zeros(max(n, 1), dtype=np.int64) for _ in range(4)]  # score, start, end, second
    proper, tlen = np.zeros(max(n // 2, 1), dtype=np.uint8), np.zeros(max(n // 2, 1), dtype=np.int64)
    per_cand = [np.zeros(max(nc, 1), dtype=np.int64) for _ in range(3)]  # score, start, end
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    tail = [cand_off.ctypes.data, cand_start.ctypes.data, cand_len.ctypes.data, cand_strand.ctypes.data, best.ctypes.data] + [a.ctypes.data for a in per_read] + \
           [proper.ctypes.data, tlen.ctypes.data] + [a.ctypes.data for a in per_cand] + [ctypes.byref(ops_p) if cigar else None, ctypes.byref(off_p) if cigar else None]
    if target is None:
        check(L.gnx_best_pair_by_offset(ctypes.byref(params), ctypes.byref(opts), n, read_cat.ctypes.data, read_off.ctypes.data, *tail))
    else:
        target = _u8(target)
        check(L.gnx_best_pair_windows(ctypes.byref(params), ctypes.byref(opts), n, read_cat.ctypes.data, read_off.ctypes.data, target.ctypes.data, target.shape[0], *tail))
    ops, off = _take(ops_p, off_p, n) if cigar else (None, None)
    return {"best": best[:n], "score": per_read[0][:n], "target_start": per_read[1][:n], "target_end": per_read[2][:n], "second_score": per_read[3][:n],
            "proper": proper[:n // 2], "tlen": tlen[:n // 2], "cand_score": per_cand[0][:nc], "cand_start": per_cand[1][:nc], "cand_end": per_cand[2][:nc],
            "ops": ops, "off": off}


def best_pair_by_offset(params, opts, read_cat, read_off, cand_off, cand_start, cand_len, cand_strand, cigar=True):
    """gnx_best_pair_by_offset: mates 2k / 2k + 1 against candidate windows of the resident reference (tables as best_of_by_offset), opts from
    pair_opts().  Returns a dict: per read best[int32], score, target_start, target_end (relative to the chosen window), second_score; per
    pair proper[uint8], tlen; per candidate cand_score, cand_start, cand_end; ops / off (None with cigar=False)."""
    return _best_pair(params, opts, read_cat, read_off, None, cand_off, cand_start, cand_len, cand_strand, cigar)


def best_pair_windows(params, opts, read_cat, read_off, target_buf, cand_off, cand_start, cand_len, cand_strand, cigar=True):
    """gnx_best_pair_windows: the same with the windows taken from target_buf."""
    return _best_pair(params, opts, read_cat, read_off, target_buf, cand_off, cand_start, cand_len, cand_strand, cigar)


# ---- candidates by seed votes (gnx_reference_index_*, gnx_seed_candidates): an index of the resident reference, reads -> candidate tables ----
def reference_index_build(seed_len, seed_step=1):
    check(lib().gnx_reference_index_build(int(seed_len), int(seed_step)))


def reference_index_info():
    """{"n_kmers", "device_bytes", "seed_len", "seed_step"} of the index of the resident reference"""
    n, b, k, s = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    check(lib().gnx_reference_index_info(ctypes.byref(n), ctypes.byref(b), ctypes.byref(k), ctypes.byref(s)))
    return {"n_kmers": n.value, "device_bytes": b.value, "seed_len": k.value, "seed_step": s.value}


def _take_array(ptr, n, ctype, dtype):
    out = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)
    lib().gnx_free(ptr)
    return out


def reference_index_get():
    """(keys, positions) of the index as uint64 arrays, sorted by key, equal keys in ascending position"""
    kp, pp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    check(lib().gnx_reference_index_get(ctypes.byref(kp), ctypes.byref(pp), ctypes.byref(n)))
    return _take_array(kp, n.value, ctypes.c_uint64, np.uint64), _take_array(pp, n.value, ctypes.c_uint64, np.uint64)


def seed_vote_opts(max_occ, bin, pad, max_cand, min_votes):
    o = GnxSeedVoteOpts()
    o.max_occ, o.bin, o.pad, o.max_cand, o.min_votes = int(max_occ), int(bin), int(pad), int(max_cand), int(min_votes)
    return o


def seed_candidates(read_cat, read_off, max_occ, bin, pad, max_cand, min_votes):
    """gnx_seed_candidates: (cand_off[n + 1], cand_start, cand_len, cand_strand, cand_votes) -- the first four are the candidate
    tables best_of_by_offset takes."""
    read_cat, read_off = _u8(read_cat), _i64(read_off)
    n = int(read_off.shape[0]) - 1
    o = seed_vote_opts(max_occ, bin, pad, max_cand, min_votes)
    ptrs = [ctypes.c_void_p() for _ in range(5)]
    check(lib().gnx_seed_candidates(ctypes.byref(o), n, read_cat.ctypes.data, read_off.ctypes.data, *[ctypes.byref(p) for p in ptrs]))
    off = _take_array(ptrs[0], n + 1, ctypes.c_int64, np.int64)
    nc = int(off[-1])
    return (off, _take_array(ptrs[1], nc, ctypes.c_int64, np.int64), _take_array(ptrs[2], nc, ctypes.c_int64, np.int64),
            _take_array(ptrs[3], nc, ctypes.c_uint8, np.uint8), _take_array(ptrs[4], nc, ctypes.c_int32, np.int32))


# ---- alignment summaries (gnx_summarize_*): CIGARs walked against their sequences on the device ----
def _ops_array(ops):
    """CIGAR runs as a contiguous CIGAR_DTYPE array (padding bytes zero); at least one element so that the pointer is never null"""
    ops = np.asarray(ops)
    out = np.zeros(max(ops.shape[0], 1), dtype=CIGAR_DTYPE)
    if ops.shape[0]:
        out["run_length"][:ops.shape[0]] = ops["run_length"]
        out["op"][:ops.shape[0]] = ops["op"]
    return out


def _summarize(call, n, xcigar, out=None):
    """call(out_ptr, xops_ref, xoff_ref) -> rc.  Returns (summaries[SUMMARY_DTYPE], xops or None, xoff or None)."""
    if out is None:
        out = np.zeros(max(n, 1), dtype=SUMMARY_DTYPE)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(call(out.ctypes.data, ctypes.byref(ops_p) if xcigar else None, ctypes.byref(off_p) if xcigar else None))
    xops, xoff = _take(ops_p, off_p, n) if xcigar else (None, None)
    return out[:n], xops, xoff


def summarize_batch_windows(params, a_buf, a_start, a_len, b_buf, b_start, b_len, ops, ops_off, xcigar=False, out=None):
    """gnx_summarize_batch_windows: the CIGARs ops[ops_off[p] : ops_off[p + 1]] walked against windows of two buffers."""
    L = lib()
    a_buf, b_buf = _u8(a_buf), _u8(b_buf)
    a_start, a_len, b_start, b_len, ops_off = _i64(a_start), _i64(a_len), _i64(b_start), _i64(b_len), _i64(ops_off)
    n, ops = int(a_start.shape[0]), _ops_array(ops)
    return _summarize(lambda o, xp, xo: L.gnx_summarize_batch_windows(ctypes.byref(params), n, a_buf.ctypes.data, a_buf.shape[0], a_start.ctypes.data, a_len.ctypes.data,
                                                                      b_buf.ctypes.data, b_buf.shape[0], b_start.ctypes.data, b_len.ctypes.data,
                                                                      ops.ctypes.data, ops_off.ctypes.data, o, xp, xo), n, xcigar, out)


def summarize_batch(params, alphas, betas, ops, ops_off, xcigar=False, out=None):
    """gnx_summarize_batch on lists of uint8 arrays."""
    L = lib()
    a_cat, a_off = _cat(list(alphas))
    b_cat, b_off = _cat(list(betas))
    n, ops, ops_off = len(alphas), _ops_array(ops), _i64(ops_off)
    return _summarize(lambda o, xp, xo: L.gnx_summarize_batch(ctypes.byref(params), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data, b_off.ctypes.data,
                                                              ops.ctypes.data, ops_off.ctypes.data, o, xp, xo), n, xcigar, out)


def summarize_batch_by_offset(params, read_cat, read_off, ref_start, ref_len, ops, ops_off, xcigar=False, out=None):
    """gnx_summarize_batch_by_offset: reads against windows of the resident reference, in the roles of best_of_by_offset."""
    L = lib()
    read_cat, read_off, ref_start, ref_len, ops_off = _u8(read_cat), _i64(read_off), _i64(ref_start), _i64(ref_len), _i64(ops_off)
    n, ops = int(ref_start.shape[0]), _ops_array(ops)
    return _summarize(lambda o, xp, xo: L.gnx_summarize_batch_by_offset(ctypes.byref(params), n, read_cat.ctypes.data, read_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                                                        ops.ctypes.data, ops_off.ctypes.data, o, xp, xo), n, xcigar, out)


# ---- MD strings (gnx_md_*) and the MAPQ rule (gnx_mapq_batch) ----
def _md(call, n):
    """call(md_ref, off_ref) -> rc.  Returns (bytes uint8[off[n]], off int64[n + 1]): pair k's string is bytes[off[k] : off[k + 1]]."""
    md_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(call(ctypes.byref(md_p), ctypes.byref(off_p)))
    off = _take_array(off_p, n + 1, ctypes.c_int64, np.int64)
    return _take_array(md_p, int(off[-1]), ctypes.c_uint8, np.uint8), off


def md_batch_windows(params, a_buf, a_start, a_len, b_buf, b_start, b_len, ops, ops_off):
    """gnx_md_batch_windows: the MD strings of the CIGARs ops[ops_off[p] : ops_off[p + 1]] against windows of two buffers (alpha is described)."""
    L = lib()
    a_buf, b_buf = _u8(a_buf), _u8(b_buf)
    a_start, a_len, b_start, b_len, ops_off = _i64(a_start), _i64(a_len), _i64(b_start), _i64(b_len), _i64(ops_off)
    n, ops = int(a_start.shape[0]), _ops_array(ops)
    return _md(lambda mp, op: L.gnx_md_batch_windows(ctypes.byref(params), n, a_buf.ctypes.data, a_buf.shape[0], a_start.ctypes.data, a_len.ctypes.data,
                                                     b_buf.ctypes.data, b_buf.shape[0], b_start.ctypes.data, b_len.ctypes.data, ops.ctypes.data, ops_off.ctypes.data, mp, op), n)


def md_batch(params, alphas, betas, ops, ops_off):
    """gnx_md_batch on lists of uint8 arrays."""
    L = lib()
    a_cat, a_off = _cat(list(alphas))
    b_cat, b_off = _cat(list(betas))
    n, ops, ops_off = len(alphas), _ops_array(ops), _i64(ops_off)
    return _md(lambda mp, op: L.gnx_md_batch(ctypes.byref(params), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data, b_off.ctypes.data,
                                             ops.ctypes.data, ops_off.ctypes.data, mp, op), n)


def md_batch_by_offset(params, read_cat, read_off, ref_start, ref_len, ops, ops_off):
    """gnx_md_batch_by_offset: reads (the queries) against windows of the resident reference (described); GNX_AFFINE_GAP_LOCAL only."""
    L = lib()
    read_cat, read_off, ref_start, ref_len, ops_off = _u8(read_cat), _i64(read_off), _i64(ref_start), _i64(ref_len), _i64(ops_off)
    n, ops = int(ref_start.shape[0]), _ops_array(ops)
    return _md(lambda mp, op: L.gnx_md_batch_by_offset(ctypes.byref(params), n, read_cat.ctypes.data, read_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                                       ops.ctypes.data, ops_off.ctypes.data, mp, op), n)


def md_strings(md, off):
    """the strings of an (md, off) pair"""
    raw = md.tobytes()
    return [raw[int(off[k]):int(off[k + 1])].decode("ascii") for k in range(off.shape[0] - 1)]


def mapq_batch(scores, second_scores):
    """gnx_mapq_batch: uint8 MAPQs from scores and second scores (INT64_MIN: no other candidate).  Host arithmetic: no device, no init."""
    scores, second_scores = _i64(scores), _i64(second_scores)
    n = int(scores.shape[0])
    out = np.zeros(max(n, 1), dtype=np.uint8)
    check(lib().gnx_mapq_batch(n, scores.ctypes.data, second_scores.ctypes.data, out.ctypes.data))
    return out[:n]


# ---- the pile of the resident reference (gnx_pileup_*) ----
def pileup_open(start, length):
    """gnx_pileup_open: a zeroed pile over [start, start + length) of the resident reference; an open one is replaced."""
    check(lib().gnx_pileup_open(int(start), int(length)))


def pileup_close():
    check(lib().gnx_pileup_close())


def pileup_info():
    """gnx_pileup_info -> {"start", "len", "reads_added", "device_bytes"}"""
    v = np.zeros(4, dtype=np.int64)
    check(lib().gnx_pileup_info(v.ctypes.data, v.ctypes.data + 8, v.ctypes.data + 16, v.ctypes.data + 24))
    return {"start": int(v[0]), "len": int(v[1]), "reads_added": int(v[2]), "device_bytes": int(v[3])}


def pileup_add_by_offset(params, read_cat, read_off, ref_start, ref_len, strand, ops, ops_off, use=None):
    """gnx_pileup_add_by_offset: reads (oriented as aligned) against windows of the resident reference, added to the open pile."""
    read_cat, read_off, ref_start, ref_len, ops_off, strand = _u8(read_cat), _i64(read_off), _i64(ref_start), _i64(ref_len), _i64(ops_off), _u8(strand)
    n, ops = int(ref_start.shape[0]), _ops_array(ops)
    if strand.shape[0] != n or (use is not None and len(use) != n):
        raise ValueError("pileup_add_by_offset: one strand byte (and one use byte) per pair")
    use = None if use is None else _u8(use)
    check(lib().gnx_pileup_add_by_offset(ctypes.byref(params), n, read_cat.ctypes.data, read_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                         strand.ctypes.data if n else None, ops.ctypes.data, ops_off.ctypes.data, None if use is None else use.ctypes.data))


def pileup_get(first=0, count=None):
    """gnx_pileup_get: rows first .. first + count of the open pile (count None: to the end of the region) as PILE_DTYPE."""
    if count is None:
        count = pileup_info()["len"] - int(first)
    out = np.zeros(max(int(count), 1), dtype=PILE_DTYPE)
    check(lib().gnx_pileup_get(int(first), int(count), out.ctypes.data))
    return out[:max(int(count), 0)]


def pileup_calls(min_depth, min_alt, frac_num, frac_den, both_strands=0):
    """gnx_pileup_calls -> PILE_CALL_DTYPE array, ordered by position"""
    o = GnxPileCallOpts(int(min_depth), int(min_alt), int(frac_num), int(frac_den), int(both_strands), 0)
    calls_p, n = ctypes.c_void_p(), ctypes.c_int64(0)
    check(lib().gnx_pileup_calls(ctypes.byref(o), ctypes.byref(calls_p), ctypes.byref(n)))
    try:
        if n.value:
            buf = (ctypes.c_char * (n.value * 24)).from_address(calls_p.value)
            return np.frombuffer(buf, dtype=PILE_CALL_DTYPE, count=n.value).copy()
        return np.zeros(0, dtype=PILE_CALL_DTYPE)
    finally:
        lib().gnx_free(calls_p)


def pileup_track_alleles(reserve=0):
    """gnx_pileup_track_alleles: the open pile, still empty, logs its indel alleles from now on; reserve sizes the first log (0: a default)."""
    check(lib().gnx_pileup_track_alleles(int(reserve)))


def pileup_allele_info():
    """gnx_pileup_allele_info -> {"tracking", "events", "device_bytes"}"""
    tr, v = np.zeros(1, dtype=np.int32), np.zeros(2, dtype=np.int64)
    check(lib().gnx_pileup_allele_info(tr.ctypes.data, v.ctypes.data, v.ctypes.data + 8))
    return {"tracking": bool(tr[0]), "events": int(v[0]), "device_bytes": int(v[1])}


def _taken(call, dtype):
    """a malloc'd array of `dtype` records that `call(byref(pointer), byref(count))` hands out, copied and freed"""
    res_p, n = ctypes.c_void_p(), ctypes.c_int64(0)
    check(call(ctypes.byref(res_p), ctypes.byref(n)))
    try:
        if n.value:
            buf = (ctypes.c_char * (n.value * dtype.itemsize)).from_address(res_p.value)
            return np.frombuffer(buf, dtype=dtype, count=n.value).copy()
        return np.zeros(0, dtype=dtype)
    finally:
        lib().gnx_free(res_p)


def pileup_alleles(normalize=False):
    """gnx_pileup_alleles (normalize: gnx_pileup_alleles_norm, every event left-normalised first) -> PILE_ALLELE_DTYPE array, ordered by
    (pos, kind, key)"""
    entry = lib().gnx_pileup_alleles_norm if normalize else lib().gnx_pileup_alleles
    return _taken(lambda p, n: entry(p, n), PILE_ALLELE_DTYPE)


def pileup_indel_calls(min_depth, min_alt, frac_num, frac_den, both_strands=0, normalize=False):
    """gnx_pileup_indel_calls (normalize: gnx_pileup_indel_calls_norm) -> PILE_INDEL_CALL_DTYPE array, in the alleles' order"""
    o = GnxPileCallOpts(int(min_depth), int(min_alt), int(frac_num), int(frac_den), int(both_strands), 0)
    entry = lib().gnx_pileup_indel_calls_norm if normalize else lib().gnx_pileup_indel_calls
    return _taken(lambda p, n: entry(ctypes.byref(o), p, n), PILE_INDEL_CALL_DTYPE)


def pileup_track_qualities(min_baseq=0):
    """gnx_pileup_track_qualities: the open pile, still empty, sums the qualities of its bases from now on; bases below min_baseq count nowhere."""
    check(lib().gnx_pileup_track_qualities(int(min_baseq)))


def pileup_qual_info():
    """gnx_pileup_qual_info -> {"tracking", "min_baseq", "device_bytes"}"""
    tr, v = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int64)
    check(lib().gnx_pileup_qual_info(tr.ctypes.data, tr.ctypes.data + 4, v.ctypes.data))
    return {"tracking": bool(tr[0]), "min_baseq": int(tr[1]), "device_bytes": int(v[0])}


def pileup_add_by_offset_qual(params, read_cat, read_off, ref_start, ref_len, strand, ops, ops_off, qual_cat, use=None):
    """gnx_pileup_add_by_offset_qual: pileup_add_by_offset with the reads' raw Phred qualities, laid out like read_cat."""
    read_cat, read_off, ref_start, ref_len, ops_off, strand = _u8(read_cat), _i64(read_off), _i64(ref_start), _i64(ref_len), _i64(ops_off), _u8(strand)
    n, ops = int(ref_start.shape[0]), _ops_array(ops)
    if strand.shape[0] != n or (use is not None and len(use) != n):
        raise ValueError("pileup_add_by_offset_qual: one strand byte (and one use byte) per pair")
    if qual_cat is not None:
        qual_cat = _u8(qual_cat)
        if qual_cat.shape[0] != read_cat.shape[0]:
            raise ValueError("pileup_add_by_offset_qual: one quality per read base")
    use = None if use is None else _u8(use)
    check(lib().gnx_pileup_add_by_offset_qual(ctypes.byref(params), n, read_cat.ctypes.data, read_off.ctypes.data, ref_start.ctypes.data, ref_len.ctypes.data,
                                              strand.ctypes.data if n else None, ops.ctypes.data, ops_off.ctypes.data, None if use is None else use.ctypes.data,
                                              None if qual_cat is None else qual_cat.ctypes.data))


def pileup_get_qual(first=0, count=None):
    """gnx_pileup_get_qual: the qsum rows first .. first + count of the open quality pile as an int32 array [count][4] (A C G T)."""
    if count is None:
        count = pileup_info()["len"] - int(first)
    out = np.zeros((max(int(count), 1), 4), dtype=np.int32)
    check(lib().gnx_pileup_get_qual(int(first), int(count), out.ctypes.data))
    return out[:max(int(count), 0)]


def pileup_genotypes(min_depth, min_qual=0, prior_het=3000, prior_hom=3300):
    """gnx_pileup_genotypes -> PILE_GENOTYPE_DTYPE array, ordered by position"""
    o = GnxGenoOpts(int(min_depth), int(min_qual), int(prior_het), int(prior_hom))
    return _taken(lambda p, n: lib().gnx_pileup_genotypes(ctypes.byref(o), p, n), PILE_GENOTYPE_DTYPE)


def pack_inserted(bases):
    """the `seq` of an insertion of at most PILE_SEQ_MAX bases: 3 bits each, code + 1 (a byte >= 4: 5), the first base lowest"""
    v = 0
    for k, b in enumerate(bases):
        v |= (min(int(b), 4) + 1) << (3 * k)
    return v


def unpack_inserted(seq):
    """the base codes of a packed `seq`"""
    out, seq = [], int(seq)
    while seq:
        out.append((seq & 7) - 1)
        seq >>= 3
    return np.asarray(out, dtype=np.uint8)


def _chunk_pairs(alphas, betas):
    n = len(alphas)
    a_off = np.zeros(n + 1, dtype=np.int64)
    b_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        a_off[1:] = np.cumsum([len(a) for a in alphas])
        b_off[1:] = np.cumsum([len(b) for b in betas])
    a_cat = _u8(np.concatenate([_u8(a) for a in alphas] + [np.zeros(1, np.uint8)]))
    b_cat = _u8(np.concatenate([_u8(b) for b in betas] + [np.zeros(1, np.uint8)]))
    return n, a_cat, a_off, b_cat, b_off, np.zeros(max(n, 1), dtype=np.int64)


def affine_gap_chunk_score_batch(params, chunk_size, alphas, betas):
    """The scores of affine_gap_chunk_batch alone (no CIGAR is built where the score sweep takes the call)."""
    n, a_cat, a_off, b_cat, b_off, scores = _chunk_pairs(alphas, betas)
    check(lib().gnx_affine_gap_chunk_score_batch(ctypes.byref(params), int(chunk_size), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data,
                                                 b_off.ctypes.data, scores.ctypes.data))
    return scores[:n]


def affine_gap_chunk_batch(params, chunk_size, alphas, betas):
    """align.AffineGapChunk over a batch of pairs.  Returns (scores, ops, off)."""
    L = lib()
    n, a_cat, a_off, b_cat, b_off, scores = _chunk_pairs(alphas, betas)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_affine_gap_chunk_batch(ctypes.byref(params), int(chunk_size), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data,
                                       b_off.ctypes.data, scores.ctypes.data, ctypes.byref(ops_p), ctypes.byref(off_p)))
    ops, off = _take(ops_p, off_p, n)
    return scores[:n], ops, off


def _group_pairs(groups, pairs):
    g = len(groups)
    blocks = [np.ascontiguousarray(x, dtype=np.uint8).reshape(x.shape[0], -1) for x in groups]
    g_off = np.zeros(g + 1, dtype=np.int64)
    if g:
        g_off[1:] = np.cumsum([b.size for b in blocks])
    g_nseq = np.asarray([b.shape[0] for b in blocks] + [0], dtype=np.int32)
    g_len = np.asarray([b.shape[1] for b in blocks] + [0], dtype=np.int64)
    bases = _u8(np.concatenate([b.reshape(-1) for b in blocks] + [np.zeros(1, np.uint8)]))
    n = len(pairs)
    pa = np.asarray([a for a, _ in pairs] + [0], dtype=np.int32)
    pb = np.asarray([b for _, b in pairs] + [0], dtype=np.int32)
    return g, bases, g_off, g_nseq, g_len, n, pa, pb, np.zeros(max(n, 1), dtype=np.int64)


def multiple_affine_gap_score_batch(params, chunk_size, groups, pairs):
    """The scores of multiple_affine_gap_batch alone (same arguments; no CIGAR is built where the score sweep takes the call)."""
    g, bases, g_off, g_nseq, g_len, n, pa, pb, scores = _group_pairs(groups, pairs)
    check(lib().gnx_multiple_affine_gap_score_batch(ctypes.byref(params), int(chunk_size), g, bases.ctypes.data, g_off.ctypes.data, g_nseq.ctypes.data,
                                                    g_len.ctypes.data, n, pa.ctypes.data, pb.ctypes.data, scores.ctypes.data))
    return scores[:n]


def multiple_affine_gap_batch(params, chunk_size, groups, pairs):
    """groups: list of 2-D uint8 arrays (nseq x len, alignment blocks); pairs: list of (a, b) group indices.
    align.multipleAffineGap (chunk_size 1) / multipleAffineGapChunk for every pair.  Returns (scores, ops, off)."""
    L = lib()
    g, bases, g_off, g_nseq, g_len, n, pa, pb, scores = _group_pairs(groups, pairs)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_multiple_affine_gap_batch(ctypes.byref(params), int(chunk_size), g, bases.ctypes.data, g_off.ctypes.data, g_nseq.ctypes.data,
                                          g_len.ctypes.data, n, pa.ctypes.data, pb.ctypes.data, scores.ctypes.data,
                                          ctypes.byref(ops_p), ctypes.byref(off_p)))
    ops, off = _take(ops_p, off_p, n)
    return scores[:n], ops, off


GNX_GSW_LEFT, GNX_GSW_RIGHT = 0, 1


def gsw_extend_batch(side, scores, gap_pen, alphas, betas):
    """genomeGraph.LeftDynamicAln / RightDynamicAln (side GNX_GSW_LEFT / GNX_GSW_RIGHT) over a batch of (target, read) pairs.
    Returns (scores, end_i, end_j, ops, off); ops are the runs in traceback order, op codes 0/1/2 = 'M'/'I'/'D'."""
    L = lib()
    n = len(alphas)
    sc = np.ascontiguousarray(np.asarray(scores, dtype=np.int64).reshape(25))
    a_off = np.zeros(n + 1, dtype=np.int64)
    b_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        a_off[1:] = np.cumsum([len(a) for a in alphas])
        b_off[1:] = np.cumsum([len(b) for b in betas])
    a_cat = _u8(np.concatenate([_u8(a) for a in alphas] + [np.zeros(1, np.uint8)]))
    b_cat = _u8(np.concatenate([_u8(b) for b in betas] + [np.zeros(1, np.uint8)]))
    out = np.zeros((3, max(n, 1)), dtype=np.int64)
    ops_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.gnx_gsw_extend_batch(int(side), sc.ctypes.data, int(gap_pen), n, a_cat.ctypes.data, a_off.ctypes.data, b_cat.ctypes.data,
                                 b_off.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                 ctypes.byref(ops_p), ctypes.byref(off_p)))
    ops, off = _take(ops_p, off_p, n)
    return out[0, :n], out[1, :n], out[2, :n], ops, off


def align_pair(params, alpha, beta):
    L = lib()
    a, b = _u8(alpha), _u8(beta)
    score = ctypes.c_int64()
    nops = ctypes.c_int64()
    ops_p = ctypes.c_void_p()
    a_ptr = a.ctypes.data if a.size else None
    b_ptr = b.ctypes.data if b.size else None
    check(L.gnx_align_pair(ctypes.byref(params), a_ptr, a.shape[0], b_ptr, b.shape[0], ctypes.byref(score), ctypes.byref(ops_p), ctypes.byref(nops)))
    total = nops.value
    if total:
        buf = (ctypes.c_char * (total * 16)).from_address(ops_p.value)
        ops = np.frombuffer(buf, dtype=CIGAR_DTYPE, count=total).copy()
    else:
        ops = np.zeros(0, dtype=CIGAR_DTYPE)
    L.gnx_free(ops_p)
    return score.value, ops


def get_timing():
    t = GnxTiming()
    check(lib().gnx_get_timing(ctypes.byref(t)))
    return {"fill_ms": t.fill_ms, "traceback_ms": t.traceback_ms, "total_ms": t.total_ms, "cells": t.cells,
            "n_launches": t.n_launches, "trace_bytes": t.trace_bytes, "dominant_ms": t.dominant_ms,
            "dominant_launches": t.dominant_launches, "fast_path": t.fast_path, "host_ms": t.host_ms, "stage0_ms": t.stage0_ms,
            "fetch_ms": t.fetch_ms, "transport": t.transport, "n_contexts": t.n_contexts, "gather_ms": t.gather_ms, "bcast_ms": t.bcast_ms}


def _cat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        off[1:] = np.cumsum([len(x) for x in seqs])
    cat = _u8(np.concatenate([_u8(x) for x in seqs] + [np.zeros(1, np.uint8)]))
    return cat, off


def seed_index_build(node_seqs, seed_len, seed_step):
    """k-mers inside nodes -> (keys uint64 sorted, locs uint64) (genomeGraph.IndexGenomeIntoMap without the node-border k-mers)"""
    L = lib()
    cat, off = _cat(node_seqs)
    kp, lp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    check(L.gnx_seed_index_build(cat.ctypes.data, off.ctypes.data, len(node_seqs), int(seed_len), int(seed_step), ctypes.byref(kp), ctypes.byref(lp), ctypes.byref(n)))
    k = n.value
    if k == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    keys = np.ctypeslib.as_array(ctypes.cast(kp, ctypes.POINTER(ctypes.c_uint64)), shape=(k,)).copy()
    locs = np.ctypeslib.as_array(ctypes.cast(lp, ctypes.POINTER(ctypes.c_uint64)), shape=(k,)).copy()
    L.gnx_free(kp)
    L.gnx_free(lp)
    return keys, locs


GIRAF_DTYPE = np.dtype([("q_start", np.int64), ("q_end", np.int64), ("t_start", np.int64), ("t_end", np.int64), ("aln_score", np.int64),
                        ("node_off", np.int64), ("n_nodes", np.int64), ("cigar_off", np.int64), ("n_cigar", np.int64),
                        ("pos_strand", np.int32), ("flag", np.int32), ("map_q", np.int32), ("has_cigar", np.int32), ("seq_is_rc", np.int32), ("panicked", np.int32)])


class GswGraph:
    """gnx_gsw_graph: nodes, edges and the seed index of a genome graph behind the C ABI (resident on the device between batches)"""

    def __init__(self, node_seqs, edges, seed_len, seed_step):
        L = lib()
        cat, off = _cat(node_seqs)
        ef = np.ascontiguousarray([u for u, _ in edges], dtype=np.int32)
        et = np.ascontiguousarray([v for _, v in edges], dtype=np.int32)
        h = ctypes.c_void_p()
        check(L.gnx_gsw_graph_create(cat.ctypes.data, off.ctypes.data, len(node_seqs), ef.ctypes.data if len(edges) else None, et.ctypes.data if len(edges) else None,
                                     len(edges), int(seed_len), int(seed_step), ctypes.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().gnx_gsw_graph_free(self._h)
            self._h = None

    __del__ = close

    def map_reads(self, read_seqs, scores, gap_pen=-600, paired=False, threads=0):
        """-> (girafs: structured array GIRAF_DTYPE, node ids uint32, cigars CIGAR_DTYPE with op = ord('M' / 'I' / 'D' / 'S'))"""
        L = lib()
        if isinstance(read_seqs, tuple):  # (bases uint8 concatenated, offsets int64[n + 1]): as the C ABI takes them
            rcat, roff = np.ascontiguousarray(read_seqs[0], dtype=np.uint8), np.ascontiguousarray(read_seqs[1], dtype=np.int64)
            if rcat.shape[0] == 0:
                rcat = np.zeros(1, np.uint8)
            n = roff.shape[0] - 1
        else:
            rcat, roff = _cat(read_seqs)
            n = len(read_seqs)
        sc = np.ascontiguousarray(scores, dtype=np.int64).reshape(25)
        gp, np_, cp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        check(L.gnx_gsw_map_reads(self._h, rcat.ctypes.data, roff.ctypes.data, n, 1 if paired else 0, sc.ctypes.data, int(gap_pen), int(threads),
                                  ctypes.byref(gp), ctypes.byref(np_), ctypes.byref(cp)))

        def take(ptr, dtype, count):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            buf = (ctypes.c_char * (count * dtype.itemsize)).from_address(ptr.value)
            return np.frombuffer(buf, dtype=dtype, count=count).copy()
        gir = take(gp, GIRAF_DTYPE, n)
        nn = int((gir["node_off"][-1] + gir["n_nodes"][-1])) if n else 0
        nc = int((gir["cigar_off"][-1] + gir["n_cigar"][-1])) if n else 0
        nodes = take(np_, np.dtype(np.uint32), nn)
        cig = take(cp, CIGAR_DTYPE, nc)
        for ptr in (gp, np_, cp):
            if ptr.value:
                L.gnx_free(ptr)
        return gir, nodes, cig


SEED_HIT_DTYPE = np.dtype([("read_start", np.int32), ("strand", np.int32), ("node", np.int32), ("node_start", np.int32), ("q_start", np.int32), ("right", np.int32)])
# The index this module uploaded last: (keys, locs, [node sequences], seed_len, generation).  The objects themselves are kept (while
# they live their ids cannot be handed to other objects) and compared by identity; whether the upload is STILL the device's resident
# index is not guessed here: the search names its generation and the library answers GNX_ESTALE when a build, another index, a graph
# handle or a shutdown took its place (gnx_seed_index_set_gen / gnx_seed_find_batch_gen) -- then it is uploaded again.
_seed_set = [None]


def _seed_resident(keys, locs, node_seqs, seed_len):
    cur = _seed_set[0]
    return (cur is not None and cur[0] is keys and cur[1] is locs and cur[3] == seed_len and len(cur[2]) == len(node_seqs)
            and all(a is b for a, b in zip(cur[2], node_seqs)))


def seed_find_batch(keys, locs, node_seqs, read_seqs, seed_len):
    """per read the list of hit tuples (read_start, strand, node, node_start, q_start, right) in the reference's order of discovery.
    The index stays resident from call to call as long as the SAME arrays come in (keys, locs and every node sequence, by identity:
    their contents must not be changed in place in between)."""
    L = lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    locs = np.ascontiguousarray(locs, dtype=np.uint64)
    seed_len = int(seed_len)
    rcat, roff = _cat(read_seqs)
    hp, op = ctypes.c_void_p(), ctypes.c_void_p()
    for attempt in range(3):
        if attempt or not _seed_resident(keys, locs, node_seqs, seed_len):
            _seed_set[0] = None
            ncat, noff = _cat(node_seqs)
            gen = ctypes.c_uint64()
            check(L.gnx_seed_index_set_gen(keys.ctypes.data, locs.ctypes.data, keys.shape[0], ncat.ctypes.data, noff.ctypes.data, len(node_seqs), seed_len, ctypes.byref(gen)))
            _seed_set[0] = (keys, locs, list(node_seqs), seed_len, gen.value)
        rc = L.gnx_seed_find_batch_gen(_seed_set[0][4], rcat.ctypes.data, roff.ctypes.data, len(read_seqs), ctypes.byref(hp), ctypes.byref(op))
        if rc != GNX_ESTALE:  # (stale again right after an upload: another thread's index got in between -- once more, then the error)
            break
    check(rc)
    off = np.ctypeslib.as_array(ctypes.cast(op, ctypes.POINTER(ctypes.c_int64)), shape=(len(read_seqs) + 1,)).copy()
    total = int(off[-1])
    if total:
        buf = (ctypes.c_char * (total * SEED_HIT_DTYPE.itemsize)).from_address(hp.value)
        hits = np.frombuffer(buf, dtype=SEED_HIT_DTYPE, count=total).copy()
    else:
        hits = np.zeros(0, dtype=SEED_HIT_DTYPE)
    if hp.value:
        L.gnx_free(hp)
    L.gnx_free(op)
    return [[tuple(int(v) for v in h) for h in hits[int(off[r]):int(off[r + 1])]] for r in range(len(read_seqs))]
