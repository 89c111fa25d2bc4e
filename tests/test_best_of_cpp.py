"""The C++ mirror of the best-of-K call (align::MapBestOf, include/gonomics_align.hpp): it compiles, refuses without a GPU, and on a
GPU reproduces the twins on the flattened pair list (tests/cpp/best_of_mirror_test.cpp: global affine and the mapping mode on both
strands with reads that have no candidates, the ties)."""
import os
import subprocess

import pytest

from gonomics_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "best_of_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "best_of_mirror_test.bin")


def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_best_of_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    rc = subprocess.call([BIN])
    assert rc in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


@pytest.mark.gpu
def test_cpp_best_of_mirror_runs():
    _build_cpp()
    assert subprocess.call([BIN]) == 0
