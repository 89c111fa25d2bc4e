"""CPU-side checks of the reference index and the seed vote (gnx_reference_index_*, gnx_seed_candidates): symbols and bindings,
every argument error (reported before the device is looked at, outputs untouched), the no-device answer, the kernels' resources,
and the restatement tests/pyref_seeds.py against cases worked out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import pyref_seeds
from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gnx_reference_index_build", "gnx_reference_index_info", "gnx_reference_index_get", "gnx_seed_candidates"]
KERNELS = ["ref_index_flag_kernel", "ref_index_emit_kernel", "ref_index_dir_kernel", "ref_seed_lookup_kernel", "ref_seed_vote_kernel<true>", "ref_seed_vote_kernel<false>", "ref_seed_windows_kernel"]


def test_symbols_exported_declared_bound_and_mirrored():
    raw = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    assert "gnx_seed_vote_opts" in hdr
    L = _lib.lib()
    for nm in ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("reference_index_build", "reference_index_info", "reference_index_get", "seed_candidates"):
        assert callable(getattr(_lib, fn))
    assert callable(align.SeedCandidates) and callable(align.MapReads) and callable(align.ReferenceIndexBuild)
    assert ctypes.sizeof(_lib.GnxSeedVoteOpts) == 32
    mirror = open(os.path.join(ROOT, "include", "gonomics_align.hpp")).read()
    for word in ("gnx_reference_index_build", "gnx_seed_candidates", "ReferenceIndexBuild", "SeedCandidates", "MapReads"):
        assert word in mirror, word


def test_new_kernels_use_no_scratch(tmp_path):
    """the kernels of both calls are in the code object, without scratch or spills; the LDS form of the vote holds its table in 7 granules"""
    import test_kernel_resources
    if not os.path.exists(test_kernel_resources.LLVM + "/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    ks = test_kernel_resources._kernels(tmp_path)
    for nm in KERNELS:
        assert nm in ks, (nm, sorted(k for k in ks if k.startswith("ref_")))
        k = ks[nm]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (nm, k)
        assert k["vgpr_count"] + k["agpr_count"] <= 64, (nm, k)  # eight waves per SIMD
        lds = 8192 if nm == "ref_seed_vote_kernel<true>" else 0  # 1024 slots of (key, votes): 7 granules of 1280 B, 18 one-wave workgroups per CU
        assert k["group_segment_fixed_size"] == lds, (nm, k)


class _Call:
    """One valid gnx_seed_candidates call (2 reads); tests break one argument at a time."""

    def __init__(self):
        self.o = _lib.seed_vote_opts(max_occ=8, bin=32, pad=16, max_cand=4, min_votes=1)
        self.reads = np.asarray(dna.StringToBases("ACGTACGTTTGCANACGTACGTAGCTAGCTAGCATCGAT"), np.uint8)
        self.read_off = np.asarray([0, 20, 39], np.int64)
        self.n = 2
        self.out = [ctypes.c_void_p() for _ in range(5)]
        self.null_out = None
        self.null_opts = self.null_reads = self.null_off = False

    def run(self):
        outs = [None if k == self.null_out else ctypes.byref(p) for k, p in enumerate(self.out)]
        return _lib.lib().gnx_seed_candidates(None if self.null_opts else ctypes.byref(self.o), self.n, None if self.null_reads else self.reads.ctypes.data,
                                              None if self.null_off else self.read_off.ctypes.data, *outs)

    def untouched(self):
        return not any(p.value for p in self.out)


def _set(field, value):
    def brk(c):
        setattr(c.o, field, value)
    brk.__name__ = "_break_%s_%s" % (field, str(value).replace("-", "m"))
    return brk


def _break_null_opts(c):
    c.null_opts = True


def _break_null_reads(c):
    c.null_reads = True


def _break_null_read_off(c):
    c.null_off = True


def _break_negative_count(c):
    c.n = -1


def _break_read_off_order(c):
    c.read_off[:] = (0, 21, 20)


def _break_read_off_start(c):
    c.read_off[0] = -1


def _null_out(k):
    def brk(c):
        c.null_out = k
    brk.__name__ = "_break_null_out_%d" % k
    return brk


BREAKS = [_break_null_opts, _break_null_reads, _break_null_read_off, _break_negative_count, _break_read_off_order, _break_read_off_start,
          _set("max_occ", 0), _set("bin", 7), _set("pad", -1), _set("max_cand", 0), _set("max_cand", 65), _set("min_votes", 0)] + [_null_out(k) for k in range(5)]


@pytest.mark.parametrize("brk", BREAKS, ids=lambda f: f.__name__[7:])
def test_argument_errors_need_no_device(brk):
    """every GNX_EINVAL of the header comment, whether or not a GPU is visible, with nothing written"""
    c = _Call()
    brk(c)
    assert c.run() == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()
    assert c.untouched()


def test_a_byte_that_is_no_base_is_refused():
    c = _Call()
    c.reads[25] = 5
    assert c.run() == _lib.GNX_EBASE
    assert c.untouched()
    with pytest.raises(IndexError):
        align.SeedCandidates([[0, 1, 2, 9]])


@pytest.mark.parametrize("k,step", [(7, 1), (33, 1), (16, 0), (16, -3), (0, 1)])
def test_index_build_argument_errors(k, step):
    assert _lib.lib().gnx_reference_index_build(k, step) == _lib.GNX_EINVAL


def test_valid_call_without_a_device_is_refused():
    """no CPU fallback: GNX_EDEVICE after the argument checks.  (With a GPU and no index built the same call answers GNX_EINVAL; the gpu
    tests check that and the results.)"""
    L = _lib.lib()
    if L.gnx_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    c = _Call()
    assert c.run() == _lib.GNX_EDEVICE
    assert c.untouched()
    c = _Call()
    c.n = 0  # also the empty batch: there is no device to ask for an index
    assert c.run() == _lib.GNX_EDEVICE and c.untouched()
    # nothing is resident without a device: no reference to index, no index to describe or copy
    assert L.gnx_reference_index_build(16, 1) == _lib.GNX_EINVAL
    assert L.gnx_reference_index_info(None, None, None, None) == _lib.GNX_EINVAL
    kp, pp, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(7)
    assert L.gnx_reference_index_get(ctypes.byref(kp), ctypes.byref(pp), ctypes.byref(n)) == _lib.GNX_EINVAL and not kp.value and not pp.value and n.value == 7
    with pytest.raises(_lib.GnxError) as ei:
        align.MapReads(_lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.DefaultScoreMatrix, -400, -30), [dna.StringToBases("ACGTACGTACGTACGTACGT")])
    assert ei.value.code == _lib.GNX_EDEVICE


# ---- the restatement against cases worked out by hand ----
def _bases(s):
    return [int(b) for b in dna.StringToBases(s)]


def test_pyref_codes_and_index():
    assert pyref_seeds.codes(_bases("ACGT"), 2) == [0b0001, 0b0110, 0b1011]  # first base most significant
    assert pyref_seeds.codes(_bases("ACNGT"), 2) == [0b0001, None, None, 0b1011]
    assert pyref_seeds.codes([0, 1, 7, 2], 2) == [1, None, None]  # a byte >= 5 spoils its k-mers like an N
    assert pyref_seeds.codes(_bases("ACG"), 4) == []
    # AAAC: AA at 0 and 1, AC at 2; equal keys in ascending position; step 2 keeps positions 0 and 2
    assert pyref_seeds.index(_bases("AAAC"), 2, 1) == [(0, 0), (0, 1), (1, 2)]
    assert pyref_seeds.index(_bases("AAAC"), 2, 2) == [(0, 0), (1, 2)]
    assert pyref_seeds.index(_bases("TNAC"), 2, 1) == [(1, 2)]
    assert pyref_seeds.revcomp(_bases("AACGN")) == _bases("NCGTT")


def test_pyref_floor_division_on_a_negative_diagonal():
    """the read's last 8 bases are the reference's first 8: t = 0, q = 4, d = -4 and floor(-4 / 8) = -1 (truncation would say 0)"""
    ref = _bases("ACGTTGCA" + "GGGGGGGGGGGGGGGGGGGGGGGG")
    read = _bases("CCCC" + "ACGTTGCA")
    tab = pyref_seeds.lookup_table(pyref_seeds.index(ref, 8, 1))
    got = pyref_seeds.candidates(len(ref), tab, 8, read, max_occ=4, bin=8, pad=2, max_cand=4, min_votes=1)
    # b = -1: start = clamp(-8 - 2) = 0, end = clamp(0 + 12 + 2) = 14.  The reverse complement TGCAACGTGGGG has no 8-mer of the reference.
    assert got == [(0, 14, 0, 1)]


def test_pyref_clamping_at_both_ends():
    ref = _bases("ACGTTGCA" + "GGGGGGGG" + "CATCATTC")  # 24 bases
    tab = pyref_seeds.lookup_table(pyref_seeds.index(ref, 8, 1))
    # d = 16, bin 8: b = 2; start = 16 - 30 -> 0; end = 24 + 8 + 30 -> 24
    assert pyref_seeds.candidates(24, tab, 8, _bases("CATCATTC"), max_occ=4, bin=8, pad=30, max_cand=4, min_votes=1) == [(0, 24, 0, 1)]
    # without padding: [16, 24 + 8) is cut at the reference end
    assert pyref_seeds.candidates(24, tab, 8, _bases("CATCATTC"), max_occ=4, bin=8, pad=0, max_cand=4, min_votes=1) == [(16, 8, 0, 1)]


def test_pyref_tie_order_max_occ_and_min_votes():
    """ACGTACGT is its own reverse complement and stands at 0 and at 16: four bins with one vote each -- strand first, then bin"""
    ref = _bases("ACGTACGT" + "GGGGGGGG" + "ACGTACGT")
    tab = pyref_seeds.lookup_table(pyref_seeds.index(ref, 8, 1))
    read = _bases("ACGTACGT")
    assert pyref_seeds.revcomp(read) == read
    full = [(0, 16, 0, 1), (16, 8, 0, 1), (0, 16, 1, 1), (16, 8, 1, 1)]
    assert pyref_seeds.candidates(24, tab, 8, read, max_occ=2, bin=8, pad=0, max_cand=4, min_votes=1) == full
    assert pyref_seeds.candidates(24, tab, 8, read, max_occ=2, bin=8, pad=0, max_cand=3, min_votes=1) == full[:3]
    assert pyref_seeds.candidates(24, tab, 8, read, max_occ=1, bin=8, pad=0, max_cand=4, min_votes=1) == []  # two entries > max_occ
    assert pyref_seeds.candidates(24, tab, 8, read, max_occ=2, bin=8, pad=0, max_cand=4, min_votes=2) == []
    # one wide bin holds both positions: two votes per strand beat everything, strand 0 first
    assert pyref_seeds.candidates(24, tab, 8, read, max_occ=2, bin=32, pad=0, max_cand=4, min_votes=2) == [(0, 24, 0, 2), (0, 24, 1, 2)]
    assert pyref_seeds.candidates(24, tab, 8, read[:7], max_occ=2, bin=8, pad=0, max_cand=4, min_votes=1) == []  # shorter than k


def test_pyref_votes_descending_come_first():
    ref = _bases("ACGTTGCAAC" + "TTTTTTTTTTTTTTTTTTTTTT" + "CGTTGCAA")  # the 8-mer CGTTGCAA at 1 and at 32
    tab = pyref_seeds.lookup_table(pyref_seeds.index(ref, 8, 1))
    got = pyref_seeds.candidates(len(ref), tab, 8, _bases("ACGTTGCAAC"), max_occ=2, bin=8, pad=0, max_cand=4, min_votes=1)
    # strand 0: q = 0, 1, 2 hit at 0, 1 (and 32), 2: diagonal 0 three times (bin 0), diagonal 31 once (bin 3).  Strand 1 (GTTGCAACGT): its
    # first 8-mer stands at 2, one vote for bin 0 -- behind strand 0's single vote for bin 3: strand decides before the bin does.
    assert got == [(0, 18, 0, 3), (24, 16, 0, 1), (0, 18, 1, 1)]
