"""Alignment summaries without a GPU: the restatement (tests/pyref_summary.py) against the oracle's scores, the C ABI's argument
checks, the SAM writer on hand-written reports, the C++ mirror's build, and the resources of the summary kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import pyref_summary as ref
import summary_cases as sc
from gonomics_amd import _lib, align, dna, sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "summary_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "summary_mirror_test.bin")


# ---- 1. the restatement re-scores the reference's own alignments to the reference's own score ----
@pytest.mark.parametrize("mode", sc.MODES)
def test_pyref_rescore_equals_the_oracle_score(mode):
    for s, (name, mx, go0, ge0) in enumerate(sc.SCORING):
        go, ge = sc.pens(mode, go0, ge0)
        alphas, betas = sc.related_pairs(mode, 500 + 10 * mode + s, 200, 60)
        for checker in ((10000, 3) if mode in (0, 1) else (10000,)):
            scores, ops, off = oracle.align_batch(mode, mx, go, ge, alphas, betas, ci=checker, cj=checker, threads=4)
            pinned = 0
            for k in range(len(alphas)):
                route = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])]
                got, x = ref.summarize(mode, mx, go, ge, alphas[k], betas[k], route)
                assert got["n_xops"] == len(x) and sum(r for r, _ in x) == sum(r for r, _ in route)
                assert got["n_equal"] + got["n_mismatch"] == sum(r for r, o in route if o == 0)
                if sc.score_is_pinned(mode, alphas[k], betas[k], checker, checker):
                    assert (got["alpha_used"], got["beta_used"]) == (len(alphas[k]), len(betas[k])), (name, mode, k)
                    assert got["rescore"] == int(scores[k]), (name, mode, checker, k, route)
                    pinned += 1
            assert pinned == len(alphas) or checker == 3


def test_pyref_on_cases_worked_out_by_hand():
    mx = align.HumanChimpTwoScoreMatrix
    a, b = dna.StringToBases("ACGTACGTAC"), dna.StringToBases("ACGAACTAC")
    s, x = ref.summarize(2, mx, -600, -150, a, b, [(6, 0), (1, 2), (3, 0)])
    assert x == [(3, 3), (1, 4), (2, 3), (1, 2), (3, 3)]
    assert s == {"rescore": 90 + 100 + 100 - 356 + 90 + 100 + 90 + 90 + 100 - 600 - 150, "alpha_used": 10, "beta_used": 9, "alpha_start": 0, "alpha_end": 10,
                 "n_equal": 8, "n_mismatch": 1, "ins_bases": 0, "del_bases": 1, "gap_runs": 1, "n_xops": 5}
    # the mapping mode: end gaps free, an I run directly behind the free D run charged as a run of its own
    s, x = ref.summarize(3, mx, -600, -150, a, dna.StringToBases("TTTACG"), [(3, 2), (2, 1), (4, 0), (3, 2)])
    assert (s["alpha_start"], s["alpha_end"], s["del_bases"], s["ins_bases"], s["gap_runs"]) == (3, 7, 0, 2, 1) and x[0] == (3, 2) and x[-1] == (3, 2)
    s, _ = ref.summarize(3, mx, -600, -150, a, [], [(4, 2), (0, 0), (3, 2)])
    assert (s["alpha_start"], s["alpha_end"], s["del_bases"], s["gap_runs"], s["rescore"], s["n_xops"], s["alpha_used"]) == (0, 0, 0, 0, 0, 1, 7)
    s, _ = ref.summarize(4, mx, -430, 0, a, [], [(4, 2), (0, 0), (3, 2)])
    assert (s["del_bases"], s["gap_runs"], s["rescore"]) == (7, 1, -430 * 7)


# ---- 2. symbols and layout ----
def test_symbols_and_struct():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in ("gnx_summarize_batch", "gnx_summarize_batch_windows", "gnx_summarize_batch_by_offset"):
        assert hasattr(L, nm) and nm in _lib.EXPORTS
    assert ctypes.sizeof(_lib.GnxAlnSummary) == 96 and _lib.SUMMARY_DTYPE.itemsize == 96
    assert [f for f, _ in _lib.GnxAlnSummary._fields_][:11] == list(ref.FIELDS) == list(_lib.SUMMARY_FIELDS)
    assert (_lib.GNX_XCOL_EQ, _lib.GNX_XCOL_X) == (3, 4) == (ref.EQ, ref.X)


# ---- 3. argument checks need no device ----
SENTINEL = 0x5A5A5A5A5A5A5A5A


class _Call:
    """one valid gnx_summarize_batch_windows call of two pairs; a test breaks one thing"""

    def __init__(self, mode=_lib.GNX_AFFINE_GAP_HIGHMEM):
        self.p = _lib.make_params(mode, align.HumanChimpTwoScoreMatrix, -600, -150)
        self.n = 2
        self.a_buf, self.b_buf = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8), np.array([0, 1, 2, 0, 1, 2, 3, 3], np.uint8)
        self.a_len_buf, self.b_len_buf = 8, 8
        self.a_start, self.a_len = np.array([0, 4], np.int64), np.array([4, 4], np.int64)
        self.b_start, self.b_len = np.array([0, 3], np.int64), np.array([3, 5], np.int64)
        self.ops, self.off = align._routes_to_ops([[(3, 0), (1, 2)], [(1, 1), (4, 0)]])
        self.out = np.full(24, SENTINEL, dtype=np.int64)
        self.null, self.want_xops, self.want_xoff = set(), False, False
        self.xops, self.xoff = ctypes.c_void_p(), ctypes.c_void_p()

    def ptr(self, name):
        return None if name in self.null else getattr(self, name).ctypes.data

    def run(self):
        L = _lib.lib()
        return L.gnx_summarize_batch_windows(None if "p" in self.null else ctypes.byref(self.p), self.n, self.ptr("a_buf"), self.a_len_buf, self.ptr("a_start"), self.ptr("a_len"),
                                             self.ptr("b_buf"), self.b_len_buf, self.ptr("b_start"), self.ptr("b_len"), self.ptr("ops"), self.ptr("off"), self.ptr("out"),
                                             ctypes.byref(self.xops) if self.want_xops else None, ctypes.byref(self.xoff) if self.want_xoff else None)

    def untouched(self):
        return bool((self.out == SENTINEL).all()) and not self.xops.value and not self.xoff.value


def _null(name):
    def brk(c):
        c.null.add(name)
    brk.__name__ = "_break_null_" + name
    return brk


def _set(attr, index, value, name):
    def brk(c):
        getattr(c, attr)[index] = value
    brk.__name__ = "_break_" + name
    return brk


def _break_negative_count(c):
    c.n = -1


def _break_mode(c):
    c.p.mode = 5


def _break_xops_only(c):
    c.want_xops = True


def _break_xoff_only(c):
    c.want_xoff = True


def _break_op3(c):
    c.ops["op"][1] = 3


def _break_negative_run(c):
    c.ops["run_length"][2] = -1


def _break_too_much_alpha(c):
    c.ops["run_length"][1] = 2   # 3 M + 2 D against 4 bases


def _break_too_much_beta(c):
    c.ops["run_length"][2] = 2   # 2 I + 4 M against 5 bases


BREAKS = [_null("p"), _null("off"), _null("out"), _null("a_start"), _null("b_len"), _null("ops"), _null("a_buf"), _break_negative_count, _break_mode, _break_xops_only, _break_xoff_only,
          _set("off", 0, 1, "ops_off_start"), _set("off", 1, 5, "ops_off_order"), _break_op3, _break_negative_run, _break_too_much_alpha, _break_too_much_beta,
          _set("a_start", 1, 5, "window_past_buffer"), _set("b_start", 0, -1, "window_start"), _set("b_len", 1, -2, "window_len")]


@pytest.mark.parametrize("brk", BREAKS, ids=lambda f: f.__name__[7:])
def test_argument_errors_need_no_device(brk):
    """every GNX_EINVAL of the header comment, whether or not a GPU is visible, with nothing written"""
    c = _Call()
    brk(c)
    assert c.run() == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()
    assert c.untouched()


def test_argument_errors_of_the_other_entries():
    L = _lib.lib()
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
    cat, off = _lib._cat([[0, 1, 2, 3]])
    ops, ooff = align._routes_to_ops([[(5, 0)]])
    out = np.full(12, SENTINEL, dtype=np.int64)
    one = np.array([4], np.int64)
    zero = np.array([0], np.int64)
    # _batch: the CIGAR consumes five bases of four
    assert L.gnx_summarize_batch(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, cat.ctypes.data, off.ctypes.data, ops.ctypes.data, ooff.ctypes.data, out.ctypes.data, None, None) == _lib.GNX_EINVAL
    assert L.gnx_summarize_batch(ctypes.byref(p), 1, cat.ctypes.data, None, cat.ctypes.data, off.ctypes.data, ops.ctypes.data, ooff.ctypes.data, out.ctypes.data, None, None) == _lib.GNX_EINVAL
    # _by_offset: the same CIGAR against the read; a null window table; a negative window
    assert L.gnx_summarize_batch_by_offset(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, zero.ctypes.data, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, out.ctypes.data, None, None) == _lib.GNX_EINVAL
    ops["run_length"][0] = 4
    assert L.gnx_summarize_batch_by_offset(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, None, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, out.ctypes.data, None, None) == _lib.GNX_EINVAL
    neg = np.array([-1], np.int64)
    assert L.gnx_summarize_batch_by_offset(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, neg.ctypes.data, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, out.ctypes.data, None, None) == _lib.GNX_EINVAL
    assert (out == SENTINEL).all()


def test_valid_call_without_a_device_is_refused():
    """no CPU fallback: GNX_EDEVICE after the argument checks (with a GPU the same call succeeds; the gpu tests check its results)"""
    has_gpu = _lib.lib().gnx_device_count() > 0
    for mode in sc.MODES:
        c = _Call(mode)
        c.want_xops = c.want_xoff = True
        rc = c.run()
        assert rc == (_lib.GNX_OK if has_gpu else _lib.GNX_EDEVICE), (mode, rc)
        if has_gpu:
            _lib.lib().gnx_free(c.xops)
            _lib.lib().gnx_free(c.xoff)
        else:
            assert c.untouched()
    if not has_gpu:
        p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.DefaultScoreMatrix, -400, -30)
        with pytest.raises(_lib.GnxError) as ei:
            align.Summarize(p, [dna.StringToBases("ACGT")], [dna.StringToBases("ACG")], [[align.Cigar(3, 0), align.Cigar(1, 2)]])
        assert ei.value.code == _lib.GNX_EDEVICE
        with pytest.raises(_lib.GnxError) as ei:
            align.MapReadsReport(p, [dna.StringToBases("ACGTACGTACGTACGTACGT")])
        assert ei.value.code == _lib.GNX_EDEVICE
    with pytest.raises(ValueError):
        align.MapReadsReport(_lib.make_params(_lib.GNX_AFFINE_GAP, align.DefaultScoreMatrix, -400, -30), [dna.StringToBases("ACGT")])
    with pytest.raises(ValueError):
        align.MapReadPairsReport(_lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.DefaultScoreMatrix, -400, -30), [dna.StringToBases("ACGT")], 0, 100)
    assert align.Summarize(c.p, [], [], []) == [] and align.FormatXCigar([(12, 3), (1, 4), (30, 3), (2, 2), (5, 3)]) == "12=1X30=2D5="


# ---- 4. the SAM writer: exact lines from hand-written reports ----
def _rep(best, strand, score, pos, xcigar, nm=(0, 0, 0), **more):
    d = {"best": best, "strand": strand, "score": score, "window_start": None if pos is None else pos - 2, "pos": pos, "end": None, "route": [], "xcigar": xcigar,
         "n_mismatch": nm[0], "ins_bases": nm[1], "del_bases": nm[2]}
    d.update(more)
    return d


def test_sam_single_reads():
    reads = [dna.StringToBases("ACGTTG"), dna.StringToBases("AACGN"), dna.StringToBases("GGGG")]
    report = [_rep(0, 0, 512, 100, [(2, 2), (3, 3), (1, 4), (1, 1), (1, 3), (40, 2)], nm=(1, 1, 0)),
              _rep(1, 1, 300, 7, [(5, 3)]),
              _rep(-1, 0, 0, None, [])]
    lines = sam.Lines(["fwd", "rev", "lost"], reads, report, "chr1", quals=["ABCDEF", "12345", "!!!!"])
    assert lines == ["fwd\t0\tchr1\t101\t255\t3=1X1I1=\t*\t0\t0\tACGTTG\tABCDEF\tAS:i:512\tNM:i:2",
                     "rev\t16\tchr1\t8\t255\t5=\t*\t0\t0\tNCGTT\t54321\tAS:i:300\tNM:i:0",
                     "lost\t4\t*\t0\t255\t*\t*\t0\t0\tGGGG\t!!!!"]
    assert sam.Lines(["fwd"], reads[:1], report[:1], "chr1")[0].split("\t")[10] == "*"


def test_sam_pairs():
    reads = [dna.StringToBases("ACGT"), dna.StringToBases("TTGA"), dna.StringToBases("CCCC"), dna.StringToBases("GGGA"), dna.StringToBases("ACAC"), dna.StringToBases("TGTG")]
    report = [_rep(0, 0, 400, 1000, [(9, 2), (4, 3)], second_score=350, proper=True, tlen=304),          # leftmost mate of a proper pair
              _rep(2, 1, 380, 1300, [(4, 3), (5, 2)], second_score=None, proper=True, tlen=304),
              _rep(0, 1, 200, 50, [(4, 3)], second_score=None, proper=False, tlen=0),                    # improper: both placed, TLEN 0
              _rep(0, 1, 210, 9000, [(3, 3), (1, 4)], nm=(1, 0, 0), second_score=-40, proper=False, tlen=0),
              _rep(0, 0, 400, 77, [(4, 3)], second_score=None, proper=False, tlen=0),                     # the mate has no placement
              _rep(-1, 0, 0, None, [], second_score=None, proper=False, tlen=0)]
    lines = sam.Lines(["p0", "p0", "p1", "p1", "p2", "p2"], reads, report, "chr2", paired=True)
    assert lines == ["p0\t99\tchr2\t1001\t255\t4=\t=\t1301\t304\tACGT\t*\tAS:i:400\tNM:i:0\tXS:i:350",
                     "p0\t147\tchr2\t1301\t255\t4=\t=\t1001\t-304\tTCAA\t*\tAS:i:380\tNM:i:0",
                     "p1\t113\tchr2\t51\t255\t4=\t=\t9001\t0\tGGGG\t*\tAS:i:200\tNM:i:0",
                     "p1\t177\tchr2\t9001\t255\t3=1X\t=\t51\t0\tTCCC\t*\tAS:i:210\tNM:i:1\tXS:i:-40",
                     "p2\t73\tchr2\t78\t255\t4=\t*\t0\t0\tACAC\t*\tAS:i:400\tNM:i:0",
                     "p2\t133\t*\t0\t255\t*\tchr2\t78\t0\tTGTG\t*"]


# ---- 5. the C++ mirror ----
def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_summary_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    assert subprocess.call([BIN]) in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


# ---- 6. kernel resources, from the gfx950 code object inside the built library ----
# name -> (VGPRs, LDS bytes) as built.  PK = 0 / 1 / 2: no side, alpha, beta read from the packed reference.
SUMMARY_PINS = {
    "aln_summary_kernel<false, 0>": (88, 0), "aln_summary_kernel<false, 1>": (92, 0), "aln_summary_kernel<false, 2>": (92, 0),
    "aln_summary_kernel<true, 0>": (90, 0), "aln_summary_kernel<true, 1>": (90, 0), "aln_summary_kernel<true, 2>": (90, 0),
    "aln_summary_bases_kernel<0>": (38, 0), "aln_summary_bases_kernel<1>": (42, 0), "aln_summary_bases_kernel<2>": (42, 0),
}


def test_summary_kernel_resources(tmp_path):
    import test_kernel_resources as tkr
    if not os.path.exists(f"{tkr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kernels = tkr._kernels(tmp_path)
    mine = {n: k for n, k in kernels.items() if n.startswith("aln_summary_")}
    assert sorted(mine) == sorted(SUMMARY_PINS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)   # no scratch, no spills
        assert k["agpr_count"] == 0, (name, k)
        assert tkr._waves_per_simd(k) >= 4, (name, k["vgpr_count"])
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == SUMMARY_PINS[name], (name, k)
