"""CPU-side checks of the best-of-K entries (gnx_best_of_*): symbols and bindings, every argument error (reported before the device
is looked at), the no-device answer, dna.ReverseComplement."""
import ctypes
import os
import re

import numpy as np
import pytest

from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gnx_best_of_by_offset", "gnx_best_of_windows"]


def test_best_of_symbols_exported_and_declared():
    raw = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    L = _lib.lib()
    for nm in ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("best_of_by_offset", "best_of_windows"):
        assert callable(getattr(_lib, fn))
    assert callable(align.MapBestOf) and callable(align.AlignBestOf) and callable(dna.ReverseComplement)
    mirror = open(os.path.join(ROOT, "include", "gonomics_align.hpp")).read()
    assert "gnx_best_of_windows" in mirror and "gnx_best_of_by_offset" in mirror and "MapBestOf" in mirror


def test_new_kernels_use_no_scratch(tmp_path):
    """the three kernels of the call are in the code object and report no scratch and no spills"""
    import test_kernel_resources
    if not os.path.exists(test_kernel_resources.LLVM + "/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    ks = test_kernel_resources._kernels(tmp_path)
    for nm in ("revcomp_reads_kernel", "first_max_kernel", "winner_tables_kernel"):
        assert nm in ks, nm
        k = ks[nm]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["group_segment_fixed_size"] == 0, (nm, k)
        assert k["vgpr_count"] + k["agpr_count"] <= 64, (nm, k)  # eight waves per SIMD


class _Call:
    """One valid gnx_best_of_windows call (2 reads, 3 candidates); tests break one argument at a time."""

    def __init__(self, mode=_lib.GNX_AFFINE_GAP):
        self.p = _lib.make_params(mode, align.DefaultScoreMatrix, -400, -30 if mode in (0, 2, 3) else 0)
        self.reads = np.asarray(dna.StringToBases("ACGTACGTTTGCA"), np.uint8)
        self.read_off = np.asarray([0, 8, 13], np.int64)
        self.target = np.asarray(dna.StringToBases("GGACGTACGTAATTGCAAACC"), np.uint8)
        self.cand_off = np.asarray([0, 2, 3], np.int64)
        self.start = np.asarray([0, 2, 9], np.int64)
        self.len = np.asarray([12, 9, 12], np.int64)
        self.strand = np.asarray([0, 1, 1], np.uint8)
        self.best = np.full(2, 77, np.int32)
        self.score = np.full(2, 77, np.int64)
        self.end = np.full(2, 77, np.int64)
        self.cand = np.full(3, 77, np.int64)
        self.ops, self.off = ctypes.c_void_p(), ctypes.c_void_p()
        self.want_end = mode == _lib.GNX_AFFINE_GAP_LOCAL
        self.want_ops, self.want_off = True, True
        self.target_len = None

    def run(self, by_offset=False):
        L = _lib.lib()
        tail = [self.cand_off.ctypes.data, self.start.ctypes.data, self.len.ctypes.data, self.strand.ctypes.data, self.best.ctypes.data, self.score.ctypes.data,
                self.end.ctypes.data if self.want_end else None, self.cand.ctypes.data,
                ctypes.byref(self.ops) if self.want_ops else None, ctypes.byref(self.off) if self.want_off else None]
        if by_offset:
            return L.gnx_best_of_by_offset(ctypes.byref(self.p), 2, self.reads.ctypes.data, self.read_off.ctypes.data, *tail)
        return L.gnx_best_of_windows(ctypes.byref(self.p), 2, self.reads.ctypes.data, self.read_off.ctypes.data, self.target.ctypes.data,
                                     self.target.shape[0] if self.target_len is None else self.target_len, *tail)

    def untouched(self):
        return bool(np.all(self.best == 77) and np.all(self.score == 77) and np.all(self.end == 77) and np.all(self.cand == 77) and not self.ops.value and not self.off.value)


def _break_cand_off_start(c):
    c.cand_off[0] = 1


def _break_cand_off_order(c):
    c.cand_off[:] = (0, 3, 2)


def _break_strand(c):
    c.strand[1] = 2


def _break_window_end(c):
    c.len[2] = 13  # 9 + 13 > 21


def _break_window_start(c):
    c.start[0] = -1


def _break_buffer_len(c):
    c.target_len = -1


def _break_ops_only(c):
    c.want_off = False


def _break_off_only(c):
    c.want_ops = False


def _break_end_in_global_mode(c):
    c.want_end = True


def _break_read_off_order(c):
    c.read_off[:] = (0, 9, 8)


def _break_mode(c):
    c.p.mode = 9


BREAKS = [_break_cand_off_start, _break_cand_off_order, _break_strand, _break_window_end, _break_window_start, _break_buffer_len, _break_ops_only, _break_off_only,
          _break_end_in_global_mode, _break_read_off_order, _break_mode]


@pytest.mark.parametrize("brk", BREAKS, ids=lambda f: f.__name__[7:])
def test_argument_errors_need_no_device(brk):
    """every GNX_EINVAL of the header comment, whether or not a GPU is visible, with nothing written"""
    c = _Call()
    brk(c)
    assert c.run() == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()
    assert c.untouched()


def test_argument_errors_of_the_resident_entry():
    for brk in (_break_cand_off_start, _break_strand, _break_ops_only, _break_end_in_global_mode):
        c = _Call()
        brk(c)
        assert c.run(by_offset=True) == _lib.GNX_EINVAL, brk.__name__
        assert c.untouched()


def test_valid_call_without_a_device_is_refused():
    """no CPU fallback: GNX_EDEVICE after the argument checks (with a GPU the same call succeeds; the gpu tests check its results)"""
    has_gpu = _lib.lib().gnx_device_count() > 0
    for mode in (_lib.GNX_AFFINE_GAP, _lib.GNX_AFFINE_GAP_LOCAL):
        c = _Call(mode)
        rc = c.run()
        assert rc == (_lib.GNX_OK if has_gpu else _lib.GNX_EDEVICE), (mode, rc)
        if has_gpu:
            _lib.lib().gnx_free(c.ops)
            _lib.lib().gnx_free(c.off)
        else:
            assert c.untouched()
    if not has_gpu:
        with pytest.raises(_lib.GnxError) as ei:
            align.MapBestOf(_lib.make_params(_lib.GNX_AFFINE_GAP, align.DefaultScoreMatrix, -400, -30), [dna.StringToBases("ACGT")], [[(dna.StringToBases("ACGTT"), 1)]])
        assert ei.value.code == _lib.GNX_EDEVICE


CASES = [("", ""), ("A", "T"), ("C", "G"), ("N", "N"), ("ACGT", "ACGT"), ("AATT", "AATT"), ("AAC", "GTT"), ("ACGTN", "NACGT"), ("GATTACA", "TGTAATC"),
         ("NNA", "TNN"), ("ACNGT", "ACNGT"), ("TTTTTTTTT", "AAAAAAAAA"), ("acgtn", "nacgt"), ("A-C", "G-T")]


@pytest.mark.parametrize("seq,rc", CASES)
def test_reverse_complement_table(seq, rc):
    got = dna.ReverseComplement(dna.StringToBases(seq))
    assert dna.BasesToString(got) == rc
    x = dna.StringToBases(seq)
    assert dna.ReverseComplement(x) is x  # in place, like the Go function


def test_reverse_complement_is_an_involution():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 3, 150, 151, 1000):
        x = rng.integers(0, 13, size=n).astype(np.uint8)
        y = dna.ReverseComplement(x.copy())
        assert y.shape == x.shape and y.dtype == np.uint8
        assert np.array_equal(dna.ReverseComplement(y.copy()), x)
        exp, up, low = x.copy(), x < 4, (x >= dna.LowerA) & (x <= dna.LowerT)
        exp[up], exp[low] = 3 - x[up], 13 - x[low]
        assert np.array_equal(y, exp[::-1])
    bad = np.asarray([0, 200, 3], np.uint8)  # a byte that is no dna.Base stays what it is
    assert dna.ReverseComplement(bad).tolist() == [0, 200, 3]
