"""CPU-side checks of the paired-end entries (gnx_best_pair_*): symbols and bindings, every argument error one at a time (reported
before the device is looked at), the no-device answer, and the selection rule's restatement (tests/pyref_pairs.py) on hand-written
tables that pin each of its clauses."""
import ctypes
import os
import re

import numpy as np
import pytest

import pyref_pairs
from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gnx_best_pair_by_offset", "gnx_best_pair_windows"]
LOCAL = _lib.GNX_AFFINE_GAP_LOCAL


def test_best_pair_symbols_exported_and_declared():
    raw = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    assert "gnx_pair_opts" in hdr
    L = _lib.lib()
    for nm in ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("best_pair_by_offset", "best_pair_windows", "pair_opts"):
        assert callable(getattr(_lib, fn))
    assert callable(align.MapBestPair) and callable(align.MapReadPairs)
    assert ctypes.sizeof(_lib.GnxPairOpts) == 32
    mirror = open(os.path.join(ROOT, "include", "gonomics_align.hpp")).read()
    assert "gnx_best_pair_windows" in mirror and "gnx_best_pair_by_offset" in mirror and "MapBestPair" in mirror and "MapReadPairs" in mirror


def test_pair_select_kernel_uses_no_scratch(tmp_path):
    """the selection kernel is in the code object, reports no scratch, no spills and no LDS, and fits eight waves per SIMD"""
    import test_kernel_resources
    if not os.path.exists(test_kernel_resources.LLVM + "/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    ks = test_kernel_resources._kernels(tmp_path)
    assert "pair_select_kernel" in ks
    k = ks["pair_select_kernel"]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] + k["agpr_count"] <= 64, k


class _Call:
    """One valid gnx_best_pair_windows call (one pair, 2 + 1 candidates); tests break one argument at a time."""

    def __init__(self):
        self.p = _lib.make_params(LOCAL, align.DefaultScoreMatrix, -400, -30)
        self.o = _lib.pair_opts(0, 100, 0)
        self.n = 2
        self.reads = np.asarray(dna.StringToBases("ACGTACGTTTGCA"), np.uint8)
        self.read_off = np.asarray([0, 8, 13], np.int64)
        self.target = np.asarray(dna.StringToBases("GGACGTACGTAATTGCAAACC"), np.uint8)
        self.cand_off = np.asarray([0, 2, 3], np.int64)
        self.start = np.asarray([0, 2, 9], np.int64)
        self.len = np.asarray([12, 9, 12], np.int64)
        self.strand = np.asarray([0, 1, 1], np.uint8)
        self.best = np.full(2, 77, np.int32)
        self.per_read = {k: np.full(2, 77, np.int64) for k in ("score", "start", "end", "second")}
        self.proper, self.tlen = np.full(1, 77, np.uint8), np.full(1, 77, np.int64)
        self.per_cand = {k: np.full(3, 77, np.int64) for k in ("score", "start", "end")}
        self.ops, self.off = ctypes.c_void_p(), ctypes.c_void_p()
        self.null = set()  # outputs passed as NULL
        self.want_ops, self.want_off = True, True
        self.target_len = None

    def _ptr(self, name, arr):
        return None if name in self.null else arr.ctypes.data

    def run(self, by_offset=False):
        L = _lib.lib()
        tail = [self.cand_off.ctypes.data, self.start.ctypes.data, self.len.ctypes.data, self.strand.ctypes.data, self._ptr("best", self.best)]
        tail += [self._ptr(k, self.per_read[k]) for k in ("score", "start", "end", "second")]
        tail += [self._ptr("proper", self.proper), self._ptr("tlen", self.tlen)]
        tail += [self._ptr("cand_" + k, self.per_cand[k]) for k in ("score", "start", "end")]
        tail += [ctypes.byref(self.ops) if self.want_ops else None, ctypes.byref(self.off) if self.want_off else None]
        head = [ctypes.byref(self.p), None if "opts" in self.null else ctypes.byref(self.o), self.n, self.reads.ctypes.data, self.read_off.ctypes.data]
        if by_offset:
            return L.gnx_best_pair_by_offset(*head, *tail)
        return L.gnx_best_pair_windows(*head, self.target.ctypes.data, self.target.shape[0] if self.target_len is None else self.target_len, *tail)

    def untouched(self):
        arrays = [self.best, self.proper, self.tlen] + list(self.per_read.values()) + list(self.per_cand.values())
        return bool(all(np.all(a == 77) for a in arrays) and not self.ops.value and not self.off.value)

    def free(self):
        _lib.lib().gnx_free(self.ops)
        _lib.lib().gnx_free(self.off)


def _break_odd_n_reads(c):
    c.n = 1


def _break_min_above_max(c):
    c.o.min_insert, c.o.max_insert = 101, 100


def _break_negative_min(c):
    c.o.min_insert = -1


def _break_negative_penalty(c):
    c.o.unpaired_penalty = -1


def _break_null_opts(c):
    c.null.add("opts")


def _break_global_mode(c):
    c.p.mode = _lib.GNX_AFFINE_GAP


def _break_unknown_mode(c):
    c.p.mode = 9


def _null(name):
    def brk(c):
        c.null.add(name)
    brk.__name__ = "_break_null_" + name
    return brk


def _break_ops_only(c):
    c.want_off = False


def _break_off_only(c):
    c.want_ops = False


def _break_strand(c):
    c.strand[1] = 2


def _break_window_end(c):
    c.len[2] = 13  # 9 + 13 > 21


def _break_window_start(c):
    c.start[0] = -1


def _break_cand_off_start(c):
    c.cand_off[0] = 1


BREAKS = [_break_odd_n_reads, _break_min_above_max, _break_negative_min, _break_negative_penalty, _break_null_opts, _break_global_mode, _break_unknown_mode,
          _null("best"), _null("score"), _null("start"), _null("end"), _null("proper"), _null("tlen"), _break_ops_only, _break_off_only, _break_strand,
          _break_window_end, _break_window_start, _break_cand_off_start]


@pytest.mark.parametrize("brk", BREAKS, ids=lambda f: f.__name__[7:])
def test_argument_errors_need_no_device(brk):
    """every GNX_EINVAL of the header comment, whether or not a GPU is visible, with nothing written"""
    c = _Call()
    brk(c)
    assert c.run() == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()
    assert c.untouched()


def test_argument_errors_of_the_resident_entry():
    for brk in (_break_odd_n_reads, _break_min_above_max, _break_negative_penalty, _break_global_mode, _null("tlen"), _break_ops_only, _break_strand):
        c = _Call()
        brk(c)
        assert c.run(by_offset=True) == _lib.GNX_EINVAL, brk.__name__
        assert c.untouched()


@pytest.mark.parametrize("optional", [(), ("second",), ("cand_score", "cand_start", "cand_end"), ("second", "cand_start")])
def test_valid_call_without_a_device_is_refused(optional):
    """no CPU fallback: GNX_EDEVICE after the argument checks, also with the optional outputs left out (with a GPU the same call
    succeeds; the gpu tests check its results)"""
    has_gpu = _lib.lib().gnx_device_count() > 0
    c = _Call()
    c.null.update(optional)
    rc = c.run()
    assert rc == (_lib.GNX_OK if has_gpu else _lib.GNX_EDEVICE), rc
    if has_gpu:
        c.free()
    else:
        assert c.untouched()
        with pytest.raises(_lib.GnxError) as ei:
            align.MapBestPair(c.p, [dna.StringToBases("ACGT"), dna.StringToBases("ACGA")], [[(0, 5, 0)], [(3, 5, 1)]], 0, 100, target=dna.StringToBases("ACGTTCGTT"))
        assert ei.value.code == _lib.GNX_EDEVICE


def test_python_wrappers_refuse_an_odd_number_of_reads():
    p = _lib.make_params(LOCAL, align.DefaultScoreMatrix, -400, -30)
    with pytest.raises(ValueError):
        align.MapBestPair(p, [dna.StringToBases("ACGT")], [[]], 0, 100)
    with pytest.raises(ValueError):
        align.MapReadPairs(p, [dna.StringToBases("ACGT")], 0, 100)
    assert align.MapBestPair(p, [], [], 0, 100) == ([], []) and align.MapReadPairs(p, [], 0, 100) == ([], [])


# ---- the restatement on hand-written tables: (score, A, E, strand) ----
F = (50, 100, 130, 0)  # the forward mate's only candidate in most cases


def _sel(m1, m2, lo=0, hi=1000, pen=0):
    return pyref_pairs.select(m1, m2, lo, hi, pen)


@pytest.mark.parametrize("E,lo,hi,proper", [(300, 200, 400, 1), (300, 200, 200, 1), (300, 201, 400, 0), (300, 100, 199, 0), (300, 100, 200, 1), (300, 0, 200, 1)])
def test_insert_bounds_are_inclusive(E, lo, hi, proper):
    """E(v) - A(f) = 200: exactly at min, exactly at max, one past each"""
    best, p, tlen, _ = _sel([F], [(40, 270, E, 1)], lo, hi)
    assert (best, p, tlen) == ((0, 0), proper, 200 if proper else 0)


def test_order_clauses():
    assert _sel([F], [(40, 100, 140, 1)])[1:3] == (1, 40)      # A(f) == A(v) is allowed
    assert _sel([F], [(40, 99, 140, 1)])[1:3] == (0, 0)        # the reverse mate starts left of the forward one
    assert _sel([F], [(40, 100, 130, 1)])[1:3] == (1, 30)      # E(f) == E(v) is allowed
    assert _sel([F], [(40, 100, 129, 1)])[1:3] == (0, 0)       # E(f) > E(v)
    assert _sel([(50, 100, 130, 1)], [(40, 90, 120, 0)])[1:3] == (1, 40)  # mate 1 on strand 1: f is mate 2's candidate
    assert _sel([(50, 100, 130, 1)], [(40, 101, 120, 0)])[1:3] == (0, 0)


def test_same_strands_and_empty_alignments_are_never_proper():
    assert _sel([F], [(40, 200, 240, 0)])[1] == 0
    assert _sel([(50, 100, 130, 1)], [(40, 200, 240, 1)])[1] == 0
    assert _sel([F], [(0, 240, 240, 1)])[1] == 0               # end == start
    assert _sel([(0, 100, 100, 0)], [(40, 200, 240, 1)])[1] == 0
    assert _sel([F], [(40, 200, 240, 1)])[1] == 1


def test_proper_wins_at_equality_and_loses_one_below():
    """mate 2's best alone (60) is improper; its proper candidate scores 45: P = 95, firstmax sum = 110"""
    m2 = [(60, 5000, 5040, 1), (45, 200, 240, 1)]
    assert _sel([F], m2, pen=15) == ((0, 1), 1, 140, (pyref_pairs.INT64_MIN, 60))   # P == U
    assert _sel([F], m2, pen=14) == ((0, 0), 0, 0, (pyref_pairs.INT64_MIN, 45))     # P == U - 1
    assert _sel([F], m2, pen=0)[0] == (0, 0) and _sel([F], m2, pen=1000)[0] == (0, 1)


def test_ties_go_to_the_lowest_c1_then_c2():
    m1 = [(50, 100, 130, 0), (50, 100, 130, 0)]
    m2 = [(40, 200, 240, 1), (40, 200, 240, 1), (40, 200, 240, 1)]
    assert _sel(m1, m2)[0] == (0, 0)
    assert _sel([(10, 100, 130, 1)] + m1, m2)[0] == (1, 0)      # the first candidate cannot pair (same strand)
    assert _sel(m1, [(40, 200, 240, 0)] + m2)[0] == (0, 1)
    assert _sel([(49, 100, 130, 0), (50, 100, 130, 0)], m2)[0] == (1, 0)


def test_a_mate_without_candidates():
    assert _sel([], [(40, 200, 240, 1), (41, 300, 340, 0)]) == ((-1, 1), 0, 0, (pyref_pairs.INT64_MIN, 40))
    assert _sel([F], []) == ((0, -1), 0, 0, (pyref_pairs.INT64_MIN, pyref_pairs.INT64_MIN))
    assert _sel([], []) == ((-1, -1), 0, 0, (pyref_pairs.INT64_MIN, pyref_pairs.INT64_MIN))


def test_runner_up_excludes_only_the_chosen_candidate():
    m1 = [(50, 100, 130, 0), (50, 900, 930, 0), (20, 0, 10, 0)]
    assert _sel(m1, [(40, 200, 240, 1)])[3] == (50, pyref_pairs.INT64_MIN)  # an equal score elsewhere is the runner-up
    best, sec, proper, tlen = pyref_pairs.select_all([m1, [(40, 200, 240, 1)], [], [F]], 0, 1000, 0)
    assert best == [0, 0, -1, 0] and proper == [1, 0] and tlen == [140, 0] and sec == [50, pyref_pairs.INT64_MIN, pyref_pairs.INT64_MIN, pyref_pairs.INT64_MIN]
