"""The alleles of the pile without a GPU: the restatement (tests/pyref_pile_alleles.py) on the header's worked values and its two
invariants against pyref_pileup, the packing pinned by hand, symbols and struct layouts, the C ABI's argument checks, the VCF text of a
hand-made call list, the C++ mirror's build, and the resources of the allele_* kernels."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import pile_allele_cases as pac
import pileup_cases as pc
import pyref_pile_alleles as ref
import test_summary_gpu as tsg
from gonomics_amd import _lib, align, dna, vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pile_alleles_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "pile_alleles_mirror_test.bin")
NAMES = ("gnx_pileup_track_alleles", "gnx_pileup_allele_info", "gnx_pileup_alleles", "gnx_pileup_indel_calls")
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _lib_built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


# ---- 1. the restatement: worked values ----
@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("region", [(100, 10), (0, 200), (103, 1), (106, 1), (104, 2), (107, 40), (90, 13)])
def test_pyref_on_the_worked_values(strand, region):
    for read, route, want in pac.WORKED:
        got = ref.add(ref.new_alleles(), pc.ALPHA_AT, dna.StringToBases(read), strand, route, region)
        inside = [w for w in want if region[0] <= w[0] < region[0] + region[1]]
        assert got == {w: [1 - strand, strand] for w in inside}, (read, region)
        assert ref.listed(got) == [w + (1, 1 - strand) for w in inside]


def test_a_deletion_is_recorded_whole_or_not_at_all():
    a = dna.StringToBases("ACGTACGTACGT")
    route = [(2, pc.M), (5, pc.D), (3, pc.M)]  # deleted: 102 .. 106
    read = a[:5]
    assert ref.events(100, read, route, (102, 1)) == [(102, ref.DEL, 5)]   # starts on the region's only position: whole, past its end
    assert ref.events(100, read, route, (103, 20)) == []                    # starts before the region, reaches in: nothing
    assert ref.events(100, read, [(2, pc.M), (2, pc.D), (0, pc.I), (3, pc.D), (3, pc.M)], (0, 200)) == [(102, ref.DEL, 5)]  # pieces are one run
    assert ref.events(100, read, [(2, pc.M), (2, pc.D), (1, pc.I), (3, pc.D), (2, pc.M)], (0, 200)) == [(102, ref.DEL, 2), (103, ref.INS, 1 + int(read[2])), (104, ref.DEL, 3)]


# ---- 2. the two invariants against pyref_pileup ----
@pytest.mark.parametrize("which", ["the_pile_seams", "the_allele_seams"])
def test_invariants_against_the_counters(which):
    g, _ = tsg._resident_cases()
    _, windows, reads, strands, routes = pc.seam_batch(g) if which == "the_pile_seams" else pac.seam_batch(g)
    for region in ((0, len(g)), (150, 3000)):
        pile, alleles = pac.restate(g, region, windows, reads, strands, routes)
        ins = [[0, 0] for _ in pile]
        dele = [[0, 0] for _ in pile]
        for (pos, kind, key), counts in alleles.items():
            assert region[0] <= pos < region[0] + region[1] and min(counts) >= 0 and sum(counts) > 0
            for s in (0, 1):
                (dele if kind == ref.DEL else ins)[pos - region[0]][s] += counts[s]
        # per position and strand: kinds 2 + 3 sum to `ins`; kind 1 never exceeds `del`
        assert ins == [r["ins"] for r in pile], region
        assert all(d[s] <= r["del"][s] for d, r in zip(dele, pile) for s in (0, 1)), region
        # (conditions on the inputs: both kinds are there, and a deletion's later columns bump `del` without an event)
        kinds = {k for _, k, _ in alleles}
        assert ref.DEL in kinds and ref.INS in kinds and sum(map(sum, dele)) < sum(sum(r["del"]) for r in pile)


# ---- 3. the packing, pinned by hand ----
def test_packing_pins():
    for bases, seq in pac.PACK_PINS:
        assert ref.pack(bases) == seq == _lib.pack_inserted(bases), bases
        assert _lib.unpack_inserted(seq).tolist() == bases
    assert ref.pack(dna.StringToBases("TT")) == 36
    top = ref.pack([3] * 21)
    assert top.bit_length() == 63 and (top << 1 | 1) < 1 << 64 and ref.pack([3] * 22).bit_length() == 66  # 21 bases and the strand bit fill the word
    a = dna.StringToBases("ACGTACGTAC")
    for n, want in ((21, (103, ref.INS, ref.pack([2] * 21))), (22, (103, ref.LONG_INS, 22))):
        read = np.concatenate([a[:4], np.full(n, 2, np.uint8), a[4:]])
        assert ref.events(100, read, [(4, pc.M), (n, pc.I), (6, pc.M)], (0, 200)) == [want]
    # a long insertion keeps its length only: two different sequences are one allele
    al = ref.new_alleles()
    for code in (1, 2):
        ref.add(al, 100, np.concatenate([a[:4], np.full(22, code, np.uint8), a[4:]]), 0, [(4, pc.M), (22, pc.I), (6, pc.M)], (0, 200))
    assert ref.listed(al) == [(103, ref.LONG_INS, 22, 2, 2)]


# ---- 4. symbols and layouts ----
def test_symbols_and_structs():
    _lib_built()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in NAMES:
        assert hasattr(L, nm) and nm in _lib.EXPORTS
    for nm in ("PileupTrackAlleles", "PileupAlleles", "PileupIndelCalls", "PileupAlleleInfo"):
        assert callable(getattr(align, nm))
    assert callable(vcf.WriteVcf)
    assert _lib.PILE_ALLELE_DTYPE.itemsize == 32 and _lib.PILE_INDEL_CALL_DTYPE.itemsize == 40
    assert [_lib.PILE_ALLELE_DTYPE.fields[f][1] for f in ("pos", "seq", "length", "count", "count_fwd", "kind")] == [0, 8, 16, 20, 24, 28]
    assert [_lib.PILE_INDEL_CALL_DTYPE.fields[f][1] for f in ("pos", "seq", "length", "count", "count_fwd", "kind", "depth", "ref")] == [0, 8, 16, 20, 24, 28, 32, 36]


# ---- 5. argument checks need no device ----
def _opts(min_depth=1, min_alt=1, num=1, den=2, both=0):
    return _lib.GnxPileCallOpts(min_depth, min_alt, num, den, both, 0)


def _indel_calls_rc(o, give_calls=True, give_n=True):
    calls, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    rc = _lib.lib().gnx_pileup_indel_calls(ctypes.byref(o) if o is not None else None, ctypes.byref(calls) if give_calls else None, ctypes.byref(n) if give_n else None)
    assert calls.value == SENTINEL and n.value == SENTINEL  # nothing was written
    return rc


@pytest.mark.parametrize("bad", [dict(min_depth=0), dict(min_depth=-3), dict(min_alt=0), dict(num=0), dict(num=-1), dict(num=3, den=2), dict(den=(1 << 20) + 1, num=1),
                                 dict(den=0, num=0), dict(both=2), dict(both=-1)], ids=str)
def test_indel_call_options_out_of_range(bad):
    _lib.check(_lib.lib().gnx_pileup_close())
    assert _indel_calls_rc(_opts(**bad)) == _lib.GNX_EINVAL
    assert b"gnx_pile_call_opts" in _lib.lib().gnx_last_error()  # (refused for the option, not for the missing pile)


def test_null_pointers_and_no_pile():
    L = _lib.lib()
    _lib.check(L.gnx_pileup_close())
    assert _indel_calls_rc(None) == _lib.GNX_EINVAL
    assert _indel_calls_rc(_opts(), give_calls=False) == _lib.GNX_EINVAL
    assert _indel_calls_rc(_opts(), give_n=False) == _lib.GNX_EINVAL
    assert _indel_calls_rc(_opts(den=1 << 20, num=1 << 20)) == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    out, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    assert L.gnx_pileup_alleles(None, ctypes.byref(n)) == _lib.GNX_EINVAL and L.gnx_pileup_alleles(ctypes.byref(out), None) == _lib.GNX_EINVAL
    assert L.gnx_pileup_alleles(ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    assert out.value == SENTINEL and n.value == SENTINEL
    for reserve in (0, 100, -1):
        assert L.gnx_pileup_track_alleles(reserve) == _lib.GNX_EINVAL
    info = np.full(3, SENTINEL, dtype=np.int64)
    assert L.gnx_pileup_allele_info(info.ctypes.data, info.ctypes.data + 8, info.ctypes.data + 16) == _lib.GNX_EINVAL and (info == SENTINEL).all()
    assert L.gnx_pileup_allele_info(None, None, None) == _lib.GNX_EINVAL
    for call in (lambda: align.PileupTrackAlleles(), lambda: align.PileupAlleles(), lambda: align.PileupIndelCalls(1, 1), lambda: align.PileupAlleleInfo()):
        with pytest.raises(_lib.GnxError) as ei:
            call()
        assert ei.value.code == _lib.GNX_EINVAL


# ---- 6. the VCF text of a hand-made call list: every record form ----
VCF_REF = "ACGTNACGTACGTTTGACCA"
VCF_TEXT = """##fileformat=VCFv4.2
##contig=<ID=chr7,length=20>
##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth at the position: read bases and deletions over it, both strands">
##INFO=<ID=AO,Number=1,Type=Integer,Description="Reads with exactly this allele">
##INFO=<ID=AOF,Number=1,Type=Integer,Description="Forward-strand share of AO">
##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Inserted bases of an <INS> whose sequence was not kept">
##ALT=<ID=INS,Description="Insertion of more than 21 bases">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
chr7\t1\t.\tACGT\tT\t.\t.\tDP=9;AO=5;AOF=2
chr7\t6\t.\tA\tG\t.\t.\tDP=12;AO=8;AOF=6
chr7\t6\t.\tACG\tA\t.\t.\tDP=10;AO=7;AOF=3
chr7\t6\t.\tA\tAT\t.\t.\tDP=12;AO=6;AOF=6
chr7\t6\t.\tA\tATNG\t.\t.\tDP=12;AO=6;AOF=0
chr7\t6\t.\tA\t<INS>\t.\t.\tDP=12;AO=7;AOF=4;SVLEN=30
chr7\t10\t.\tACG\tA\t.\t.\tDP=20;AO=11;AOF=5
chr7\t10\t.\tACGTT\tA\t.\t.\tDP=20;AO=9;AOF=4
chr7\t20\t.\tA\tC\t.\t.\tDP=4;AO=4;AOF=1
chr7\t20\t.\tA\tAA\t.\t.\tDP=4;AO=3;AOF=1
"""


def _vcf_calls():
    subs = [{"pos": 5, "depth": 12, "count": 8, "count_fwd": 6, "kind": "sub", "ref": 0, "alt": 2},
            {"pos": 10, "depth": 20, "count": 20, "count_fwd": 9, "kind": "del", "ref": 1, "alt": None},   # PileupCalls' own indel lines: not written
            {"pos": 5, "depth": 12, "count": 19, "count_fwd": 10, "kind": "ins", "ref": 0, "alt": None},
            {"pos": 19, "depth": 4, "count": 4, "count_fwd": 1, "kind": "sub", "ref": 0, "alt": 1}]

    def al(pos, kind, length, seq, depth, count, fwd, refc):
        return {"pos": pos, "kind": kind, "length": length, "seq": None if seq is None else dna.StringToBases(seq), "count": count, "count_fwd": fwd, "depth": depth, "ref": refc}

    indels = [al(0, "del", 3, None, 9, 5, 2, 0),            # a deletion at x == 0: anchored behind
              al(5, "ins", 1, "T", 12, 6, 6, 0), al(5, "ins", 3, "TNG", 12, 6, 0, 0), al(5, "long_ins", 30, None, 12, 7, 4, 0),
              al(6, "del", 2, None, 10, 7, 3, 1),           # POS 6 as well: behind the substitution there, before the insertions
              al(10, "del", 2, None, 20, 11, 5, 1), al(10, "del", 4, None, 20, 9, 4, 1),
              al(19, "ins", 1, "A", 4, 3, 1, 0)]
    return subs, indels


@pytest.mark.parametrize("as_callable", [False, True])
def test_vcf_text(as_callable):
    codes = dna.StringToBases(VCF_REF)
    subs, indels = _vcf_calls()
    out = io.StringIO()
    n = vcf.WriteVcf(out, "chr7", (lambda start, k: codes[start:start + k]) if as_callable else codes, subs, indels)
    want = VCF_TEXT.replace("##contig=<ID=chr7,length=20>", "##contig=<ID=chr7>") if as_callable else VCF_TEXT
    assert out.getvalue() == want and n == 10
    recs = pac.parse_vcf(out.getvalue())
    assert [r[1] for r in recs] == sorted(r[1] for r in recs) and {"<INS>"} < {r[3] for r in recs}


# ---- 7. the C++ mirror ----
def _build_cpp():
    _lib_built()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_pile_alleles_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    assert subprocess.call([BIN]) in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


# ---- 8. kernel resources, from the gfx950 code object inside the built library ----
# name -> (VGPRs, LDS bytes) as built
ALLELE_PINS = {"allele_log_kernel": (68, 0), "allele_reduce_kernel<false>": (30, 0), "allele_reduce_kernel<true>": (38, 0),
               "allele_call_kernel<false>": (40, 0), "allele_call_kernel<true>": (44, 0)}


def test_allele_kernel_resources(tmp_path):
    import test_kernel_resources as tkr
    if not os.path.exists(f"{tkr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kernels = tkr._kernels(tmp_path)
    mine = {n: k for n, k in kernels.items() if n.startswith("allele_")}
    assert sorted(mine) == sorted(ALLELE_PINS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)   # no scratch, no spills
        assert k["agpr_count"] == 0, (name, k)
        assert tkr._waves_per_simd(k) >= 4, (name, k["vgpr_count"])
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == ALLELE_PINS[name], (name, k)
