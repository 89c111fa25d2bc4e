"""MD strings and the MAPQ rule without a GPU: the restatement (tests/pyref_md.py) on the header's worked values and against the summary's
counts, gnx_mapq_batch (host arithmetic), the C ABI's argument checks, the SAM writer on hand-written reports, the C++ mirror's build,
and the resources of the aln_md_* kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import md_cases as mc
import oracle
import pyref_md as ref
import pyref_summary
import summary_cases as sc
import test_summary_cpu as tsc
from gonomics_amd import _lib, align, dna, sam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "md_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "md_mirror_test.bin")
NAMES = ("gnx_md_batch", "gnx_md_batch_windows", "gnx_md_batch_by_offset", "gnx_mapq_batch")


# ---- 1. the restatement: worked values and the three invariants ----
def test_pyref_on_the_worked_values():
    alpha = dna.StringToBases(mc.ALPHA)
    for mode, beta, route, md in mc.WORKED:
        assert ref.md(mode, alpha, dna.StringToBases(beta), route) == md, (mode, beta)
    (case,) = [c for c in sc.seam_cases() if c[0] == "m63_64_65"]
    for mode in sc.MODES:
        assert ref.md(mode, case[1], case[2], case[3]) == mc.M63_64_65
    alpha, beta, route = mc.digit_boundary()
    assert 11000 < sum(r for r, _ in route) < 13000
    for mode in sc.MODES:
        assert ref.md(mode, alpha, beta, route) == mc.digit_boundary_md()


def _check_invariants(mode, alpha, beta, route, what):
    text = ref.md(mode, alpha, beta, route)
    assert ref.PATTERN.fullmatch(text), (what, text)
    s, _ = pyref_summary.summarize(mode, align.HumanChimpTwoScoreMatrix, -600, -150, alpha, beta, route)
    assert ref.parts(text) == (s["n_equal"], s["n_mismatch"], s["del_bases"]), (what, text, s)
    return text


@pytest.mark.parametrize("mode", sc.MODES)
def test_invariants_against_the_summary(mode):
    for name, alpha, beta, route in sc.seam_cases():
        _check_invariants(mode, alpha, beta, route, (name, mode))
    for extra in (mc.digit_boundary(), mc.d_group()):
        _check_invariants(mode, *extra, what=mode)
    name, mx, go0, ge0 = sc.SCORING[0]
    go, ge = sc.pens(mode, go0, ge0)
    alphas, betas = sc.related_pairs(mode, 500 + 10 * mode, 200, 60)
    _, ops, off = oracle.align_batch(mode, mx, go, ge, alphas, betas, ci=10000, cj=10000, threads=4)
    texts = []
    for k in range(len(alphas)):
        route = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])]
        texts.append(_check_invariants(mode, alphas[k], betas[k], route, (mode, k)))
    assert any("^" in t for t in texts) and any(t != "0" and not t.isdigit() for t in texts)  # (the inputs do hold events)


# ---- 2. the MAPQ rule: host arithmetic, no device ----
def test_mapq_pins():
    none = np.iinfo(np.int64).min
    scores = [s for s, _, _ in mc.MAPQ_PINS]
    seconds = [s2 for _, s2, _ in mc.MAPQ_PINS]
    want = [q for _, _, q in mc.MAPQ_PINS]
    assert [ref.mapq(s, s2) for s, s2 in zip(scores, seconds)] == want
    assert _lib.mapq_batch(scores, [none if s2 is None else s2 for s2 in seconds]).tolist() == want
    assert align.Mapq(scores, seconds) == want and align.Mapq([], []) == []
    # the edges of int64, and a sweep against the restatement
    big = np.iinfo(np.int64).max
    assert align.Mapq([big, big, big, big], [None, big - 1, big // 2, 1]) == [60, 0, 30, 59] == [ref.mapq(big, x) for x in (None, big - 1, big // 2, 1)]
    rng = np.random.default_rng(5)
    s = [int(x) for x in rng.integers(-50, 2000, size=400)] + [int(x) for x in rng.integers(1 << 61, (1 << 63) - 1, size=100)]
    s2 = [min(big, int(rng.random() * (max(v, 1) + 150)) - 100) for v in s]
    assert align.Mapq(s, s2) == [ref.mapq(a, b) for a, b in zip(s, s2)]
    L = _lib.lib()
    one = np.zeros(1, np.int64)
    q = np.full(1, 0x5A, np.uint8)
    assert L.gnx_mapq_batch(-1, one.ctypes.data, one.ctypes.data, q.ctypes.data) == _lib.GNX_EINVAL
    for broken in range(3):
        ptrs = [one.ctypes.data, one.ctypes.data, q.ctypes.data]
        ptrs[broken] = None
        assert L.gnx_mapq_batch(1, *ptrs) == _lib.GNX_EINVAL
    assert q[0] == 0x5A and L.gnx_mapq_batch(0, None, None, None) == _lib.GNX_OK


# ---- 3. symbols ----
def test_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in NAMES:
        assert hasattr(L, nm) and nm in _lib.EXPORTS
    for nm in ("MDTags", "MDTagsByOffset", "Mapq"):
        assert callable(getattr(align, nm))


# ---- 4. argument checks need no device: the summary's break list against the MD twin ----
class _MdCall(tsc._Call):
    """the valid gnx_summarize_batch_windows call of test_summary_cpu as a gnx_md_batch_windows call: the two required outputs stand where
    out / out_xops / out_xops_off stand (a break that withholds one of those withholds one of these)"""

    def run(self):
        L = _lib.lib()
        no_md = "out" in self.null or (self.want_xoff and not self.want_xops)
        no_off = "out" in self.null or (self.want_xops and not self.want_xoff)
        return L.gnx_md_batch_windows(None if "p" in self.null else ctypes.byref(self.p), self.n, self.ptr("a_buf"), self.a_len_buf, self.ptr("a_start"), self.ptr("a_len"),
                                      self.ptr("b_buf"), self.b_len_buf, self.ptr("b_start"), self.ptr("b_len"), self.ptr("ops"), self.ptr("off"),
                                      None if no_md else ctypes.byref(self.xops), None if no_off else ctypes.byref(self.xoff))

    def untouched(self):
        return not self.xops.value and not self.xoff.value


@pytest.mark.parametrize("brk", tsc.BREAKS, ids=lambda f: f.__name__[7:])
def test_argument_errors_need_no_device(brk):
    c = _MdCall()
    brk(c)
    assert c.run() == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()
    assert c.untouched()


def test_argument_errors_of_the_other_entries():
    L = _lib.lib()
    cat, off = _lib._cat([[0, 1, 2, 3]])
    ops, ooff = align._routes_to_ops([[(4, 0)]])
    one, zero = np.array([4], np.int64), np.array([0], np.int64)
    md, moff = ctypes.c_void_p(), ctypes.c_void_p()
    refs = (ctypes.byref(md), ctypes.byref(moff))
    for mode in sc.MODES:  # _by_offset: the window is the described side in the mapping mode only
        p = _lib.make_params(mode, align.HumanChimpTwoScoreMatrix, -600, -150)
        rc = L.gnx_md_batch_by_offset(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, zero.ctypes.data, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, *refs)
        if mode != sc.LOCAL:
            assert rc == _lib.GNX_EINVAL, mode
    p = _lib.make_params(sc.LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
    assert L.gnx_md_batch_by_offset(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, None, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, *refs) == _lib.GNX_EINVAL
    assert L.gnx_md_batch_by_offset(None, 1, cat.ctypes.data, off.ctypes.data, zero.ctypes.data, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, *refs) == _lib.GNX_EINVAL
    ops["run_length"][0] = 5  # the CIGAR consumes five bases of four
    assert L.gnx_md_batch_by_offset(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, zero.ctypes.data, one.ctypes.data, ops.ctypes.data, ooff.ctypes.data, *refs) == _lib.GNX_EINVAL
    assert L.gnx_md_batch(ctypes.byref(p), 1, cat.ctypes.data, off.ctypes.data, cat.ctypes.data, off.ctypes.data, ops.ctypes.data, ooff.ctypes.data, *refs) == _lib.GNX_EINVAL
    assert L.gnx_md_batch(ctypes.byref(p), 1, cat.ctypes.data, None, cat.ctypes.data, off.ctypes.data, ops.ctypes.data, ooff.ctypes.data, *refs) == _lib.GNX_EINVAL
    assert not md.value and not moff.value


def test_valid_call_without_a_device_is_refused():
    """no CPU fallback: GNX_EDEVICE after the argument checks (with a GPU the same call succeeds; the gpu tests check its bytes)"""
    has_gpu = _lib.lib().gnx_device_count() > 0
    for mode in sc.MODES:
        c = _MdCall(mode)
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
            align.MDTags(p, [dna.StringToBases("ACGT")], [dna.StringToBases("ACG")], [[align.Cigar(3, 0), align.Cigar(1, 2)]])
        assert ei.value.code == _lib.GNX_EDEVICE
        with pytest.raises(_lib.GnxError) as ei:
            align.MapReadsReport(p, [dna.StringToBases("ACGTACGTACGTACGTACGT")], tags=True)
        assert ei.value.code == _lib.GNX_EDEVICE
    assert align.MDTags(c.p, [], [], []) == [] and align.MDTagsByOffset(c.p, [], [], []) == []


# ---- 5. the SAM writer: exact lines from hand-written reports with md / mapq ----
def test_sam_single_reads_with_tags():
    reads = [dna.StringToBases("ACGTTG"), dna.StringToBases("AACGN"), dna.StringToBases("GGGG")]
    report = [tsc._rep(0, 0, 512, 100, [(2, 2), (3, 3), (1, 4), (1, 1), (1, 3), (40, 2)], nm=(1, 1, 0), md="3A1", mapq=37, second_score=200),
              tsc._rep(1, 1, 300, 7, [(5, 3)], md="5", mapq=60, second_score=None),
              tsc._rep(-1, 0, 0, None, [], md=None, mapq=0, second_score=None)]
    lines = sam.Lines(["fwd", "rev", "lost"], reads, report, "chr1", quals=["ABCDEF", "12345", "!!!!"])
    assert lines == ["fwd\t0\tchr1\t101\t37\t3=1X1I1=\t*\t0\t0\tACGTTG\tABCDEF\tAS:i:512\tNM:i:2\tMD:Z:3A1\tXS:i:200",
                     "rev\t16\tchr1\t8\t60\t5=\t*\t0\t0\tNCGTT\t54321\tAS:i:300\tNM:i:0\tMD:Z:5",
                     "lost\t4\t*\t0\t255\t*\t*\t0\t0\tGGGG\t!!!!"]
    # md alone, mapq alone, neither: each key acts on its own, and a report without them writes today's line
    only_md = sam.Lines(["fwd"], reads[:1], [tsc._rep(0, 0, 512, 100, [(6, 3)], md="6")], "chr1")[0].split("\t")
    assert only_md[4] == "255" and only_md[11:] == ["AS:i:512", "NM:i:0", "MD:Z:6"]
    only_q = sam.Lines(["fwd"], reads[:1], [tsc._rep(0, 0, 512, 100, [(6, 3)], mapq=0)], "chr1")[0].split("\t")
    assert only_q[4] == "0" and only_q[11:] == ["AS:i:512", "NM:i:0"]
    assert sam.Lines(["fwd"], reads[:1], [tsc._rep(0, 0, 512, 100, [(6, 3)])], "chr1") == ["fwd\t0\tchr1\t101\t255\t6=\t*\t0\t0\tACGTTG\t*\tAS:i:512\tNM:i:0"]


def test_sam_pairs_with_tags():
    reads = [dna.StringToBases("ACGT"), dna.StringToBases("TTGA"), dna.StringToBases("ACAC"), dna.StringToBases("TGTG")]
    report = [tsc._rep(0, 0, 400, 1000, [(9, 2), (4, 3)], second_score=350, proper=True, tlen=304, md="4", mapq=7),
              tsc._rep(2, 1, 380, 1300, [(3, 3), (1, 2), (1, 3), (5, 2)], nm=(0, 0, 1), second_score=None, proper=True, tlen=304, md="3^C1", mapq=60),
              tsc._rep(0, 0, 400, 77, [(2, 3), (1, 4), (1, 3)], nm=(1, 0, 0), second_score=-40, proper=False, tlen=0, md="2N1", mapq=60),
              tsc._rep(-1, 0, 0, None, [], second_score=None, proper=False, tlen=0, md=None, mapq=0)]
    lines = sam.Lines(["p0", "p0", "p2", "p2"], reads, report, "chr2", paired=True)
    assert lines == ["p0\t99\tchr2\t1001\t7\t4=\t=\t1301\t304\tACGT\t*\tAS:i:400\tNM:i:0\tMD:Z:4\tXS:i:350",
                     "p0\t147\tchr2\t1301\t60\t3=1D1=\t=\t1001\t-304\tTCAA\t*\tAS:i:380\tNM:i:1\tMD:Z:3^C1",
                     "p2\t73\tchr2\t78\t60\t2=1X1=\t*\t0\t0\tACAC\t*\tAS:i:400\tNM:i:1\tMD:Z:2N1\tXS:i:-40",
                     "p2\t133\t*\t0\t255\t*\tchr2\t78\t0\tTGTG\t*"]


# ---- 6. the C++ mirror ----
def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_md_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    assert subprocess.call([BIN]) in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


# ---- 7. kernel resources, from the gfx950 code object inside the built library ----
# name -> (VGPRs, LDS bytes) as built.  <WRITE, PK>; PK = 0 / 1 / 2: no side, alpha, beta read from the packed reference.
MD_PINS = {
    "aln_md_kernel<false, 0>": (86, 0), "aln_md_kernel<false, 1>": (82, 0), "aln_md_kernel<false, 2>": (82, 0),
    "aln_md_kernel<true, 0>": (95, 0), "aln_md_kernel<true, 1>": (88, 0), "aln_md_kernel<true, 2>": (90, 0),
}


def test_md_kernel_resources(tmp_path):
    import test_kernel_resources as tkr
    if not os.path.exists(f"{tkr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kernels = tkr._kernels(tmp_path)
    mine = {n: k for n, k in kernels.items() if n.startswith("aln_md_")}
    assert sorted(mine) == sorted(MD_PINS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)   # no scratch, no spills
        assert k["agpr_count"] == 0, (name, k)
        assert tkr._waves_per_simd(k) >= 4, (name, k["vgpr_count"])
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == MD_PINS[name], (name, k)
