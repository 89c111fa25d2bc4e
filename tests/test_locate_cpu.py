"""CPU-side checks of the locate entries (gnx_locate_*): symbols and bindings, the no-device and wrong-mode errors, the C++ mirror's
build.  The resources of the local score sweep's kernels: test_kernel_resources.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCATE_ENTRIES = ["gnx_locate_batch", "gnx_locate_batch_windows", "gnx_locate_batch_by_offset"]
SRC = os.path.join(ROOT, "tests", "cpp", "locate_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "locate_mirror_test.bin")


def test_locate_symbols_exported_and_declared():
    raw = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    L = _lib.lib()
    for nm in LOCATE_ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("locate_batch", "locate_batch_windows", "locate_batch_by_offset"):
        assert callable(getattr(_lib, fn))
    for fn in ("LocateBatch", "AffineGapLocalEnd"):
        assert callable(getattr(align, fn))
    field = re.search(r"int32_t fast_path;.*?\*/", raw, flags=re.S).group(0)
    assert "7" in field and "8" in field


def test_locate_errors_without_a_device_and_with_a_global_mode():
    L = _lib.lib()
    t, q = dna.StringToBases("ACGTACGT"), dna.StringToBases("ACG")
    if L.gnx_device_count() > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    with pytest.raises(_lib.GnxError) as ei:
        align.AffineGapLocalEnd(t, q, align.DefaultScoreMatrix, -400, -30)
    assert ei.value.code == _lib.GNX_EDEVICE
    for mode in (_lib.GNX_AFFINE_GAP, _lib.GNX_CONST_GAP, _lib.GNX_AFFINE_GAP_HIGHMEM, _lib.GNX_CONST_GAP_HIGHMEM):
        with pytest.raises(_lib.GnxError) as ei:
            _lib.locate_batch(_lib.make_params(mode, align.DefaultScoreMatrix, -400, -30 if mode in (0, 2) else 0), [np.asarray(t)], [np.asarray(q)])
        assert ei.value.code == _lib.GNX_EINVAL, mode


def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_locate_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    rc = subprocess.call([BIN])
    assert rc in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box
