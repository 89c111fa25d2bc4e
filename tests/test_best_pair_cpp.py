"""The C++ mirror of the paired-end call (align::MapBestPair, include/gonomics_align.hpp): it compiles, refuses without a GPU, and on a
GPU gives, field by field, what the ctypes call gives on the same tables (tests/cpp/best_pair_mirror_test.cpp reads them from a file)."""
import os
import subprocess

import numpy as np
import pytest

from gonomics_amd import _lib, align

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "best_pair_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "best_pair_mirror_test.bin")


def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_best_pair_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    rc = subprocess.call([BIN])
    assert rc in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


@pytest.mark.gpu
@pytest.mark.parametrize("cigar", [True, False])
def test_cpp_best_pair_mirror_equals_ctypes(gpu_lib, tmp_path, cigar):
    import test_best_pair_gpu as T
    reads, target, cands, _ = T._fuzz()
    lo, hi, pen, go, ge = T.LO, T.HI, T.PEN, T.GO, T.GE
    words = [lo, hi, pen, go, ge, int(cigar), len(reads), len(target)] + target.tolist()
    for rd, cs in zip(reads, cands):
        words += [len(rd)] + rd.tolist() + [len(cs)] + [x for c in cs for x in c]
    path = tmp_path / "tables.txt"
    path.write_text(" ".join(str(int(w)) for w in words))
    _build_cpp()
    out = subprocess.run([BIN, str(path)], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    got = T._call(gpu_lib, gpu_lib.make_params(T.LOCAL, align.DefaultScoreMatrix, go, ge), reads, target, cands, lo, hi, pen, cigar=cigar)
    lines, c_off = [], np.concatenate([[0], np.cumsum([len(c) for c in cands])])
    flat_start = [c[0] for cs in cands for c in cs]
    for r in range(len(reads)):
        b, sec = int(got["best"][r]), int(got["second_score"][r])
        has = sec != np.iinfo(np.int64).min
        head = [b, got["score"][r], got["target_start"][r], got["target_end"][r], flat_start[c_off[r] + b] if b >= 0 else 0, int(has), sec if has else 0]
        cand = [x for c in range(c_off[r], c_off[r + 1]) for x in (got["cand_score"][c], got["cand_start"][c], got["cand_end"][c])]
        route = [x for k in range(got["off"][r], got["off"][r + 1]) for x in (got["ops"]["run_length"][k], got["ops"]["op"][k])] if cigar else []
        lines.append(" ".join(["read"] + [str(int(x)) for x in head] + ["cand"] + [str(int(x)) for x in cand] + ["route"] + [str(int(x)) for x in route]))
    lines += ["pair %d %d" % (int(p), int(t)) for p, t in zip(got["proper"], got["tlen"])]
    assert [ln.strip() for ln in out.stdout.strip().split("\n")] == [ln.strip() for ln in lines]
