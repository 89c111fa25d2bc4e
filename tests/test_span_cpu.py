"""CPU-side checks of the span entries (gnx_locate_span_*): symbols and bindings, argument errors, the lemma the route
rests on (checked on the oracle alone), the scalar model of the stage-2 kernel against the oracle, the kernel's resources read from the
code object, and the C++ mirror's build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import common
import oracle
import pyref_span
from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SPAN_ENTRIES = ["gnx_locate_span_batch", "gnx_locate_span_batch_windows", "gnx_locate_span_batch_by_offset"]
SRC = os.path.join(ROOT, "tests", "cpp", "span_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "span_mirror_test.bin")


def test_span_symbols_exported_and_declared():
    raw = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(gnx_[a-z_]+)\s*\(", hdr))
    L = _lib.lib()
    for nm in SPAN_ENTRIES:
        assert nm in declared, nm
        assert nm in _lib.EXPORTS, nm
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), nm), nm
        assert getattr(L, nm).restype is ctypes.c_int and getattr(L, nm).argtypes, nm
    for fn in ("locate_span_batch", "locate_span_batch_windows", "locate_span_batch_by_offset"):
        assert callable(getattr(_lib, fn))
    for fn in ("LocateSpanBatch", "AffineGapLocalSpan"):
        assert callable(getattr(align, fn))
    field = re.search(r"int32_t fast_path;.*?\*/", raw, flags=re.S).group(0)
    assert re.search(r"\b10:", field), field


def _raw_call(L, params, t, q, score=True, start=True, end=True):
    """gnx_locate_span_batch on one pair with chosen output pointers left null."""
    t_off = np.asarray([0, len(t)], dtype=np.int64)
    q_off = np.asarray([0, len(q)], dtype=np.int64)
    t, q = np.ascontiguousarray(t, dtype=np.uint8), np.ascontiguousarray(q, dtype=np.uint8)
    out = [np.full(1, -7, dtype=np.int64) for _ in range(3)]
    ptr = [o.ctypes.data if use else None for o, use in zip(out, (score, start, end))]
    rc = L.gnx_locate_span_batch(ctypes.byref(params), 1, t.ctypes.data, t_off.ctypes.data, q.ctypes.data, q_off.ctypes.data, *ptr)
    return rc, out


def test_span_argument_errors():
    L = _lib.lib()
    t, q = np.asarray(dna.StringToBases("ACGTACGT")), np.asarray(dna.StringToBases("ACG"))
    local = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.DefaultScoreMatrix, -400, -30)
    # every global mode is refused, on any machine, before anything is written
    for mode in (_lib.GNX_AFFINE_GAP, _lib.GNX_CONST_GAP, _lib.GNX_AFFINE_GAP_HIGHMEM, _lib.GNX_CONST_GAP_HIGHMEM):
        p = _lib.make_params(mode, align.DefaultScoreMatrix, -400, -30 if mode in (0, 2) else 0)
        with pytest.raises(_lib.GnxError) as ei:
            _lib.locate_span_batch(p, [t], [q])
        assert ei.value.code == _lib.GNX_EINVAL, mode
        rc, out = _raw_call(L, p, t, q)
        assert rc == _lib.GNX_EINVAL and all(int(o[0]) == -7 for o in out), mode
    # each output vector is required
    for k in range(3):
        use = [True, True, True]
        use[k] = False
        rc, _ = _raw_call(L, local, t, q, *use)
        assert rc == _lib.GNX_EINVAL, k
    # what the locate twin refuses, the span entry refuses with the same code: null tables, a negative count, windows out of bounds
    z = np.zeros(2, dtype=np.int64)
    o3 = [np.zeros(1, dtype=np.int64) for _ in range(3)]
    assert L.gnx_locate_batch(ctypes.byref(local), 1, t.ctypes.data, None, q.ctypes.data, z.ctypes.data, o3[0].ctypes.data, o3[2].ctypes.data) == _lib.GNX_EINVAL
    assert L.gnx_locate_span_batch(ctypes.byref(local), 1, t.ctypes.data, None, q.ctypes.data, z.ctypes.data, *[o.ctypes.data for o in o3]) == _lib.GNX_EINVAL
    assert L.gnx_locate_span_batch(ctypes.byref(local), 1, t.ctypes.data, z.ctypes.data, q.ctypes.data, None, *[o.ctypes.data for o in o3]) == _lib.GNX_EINVAL
    assert L.gnx_locate_batch(ctypes.byref(local), -1, t.ctypes.data, z.ctypes.data, q.ctypes.data, z.ctypes.data, o3[0].ctypes.data, o3[2].ctypes.data) == _lib.GNX_EINVAL
    assert L.gnx_locate_span_batch(ctypes.byref(local), -1, t.ctypes.data, z.ctypes.data, q.ctypes.data, z.ctypes.data, *[o.ctypes.data for o in o3]) == _lib.GNX_EINVAL
    assert L.gnx_locate_span_batch_by_offset(ctypes.byref(local), 1, q.ctypes.data, z.ctypes.data, None, None, *[o.ctypes.data for o in o3]) == _lib.GNX_EINVAL
    assert L.gnx_locate_span_batch_by_offset(ctypes.byref(local), 1, q.ctypes.data, None, z.ctypes.data, z.ctypes.data, *[o.ctypes.data for o in o3]) == _lib.GNX_EINVAL
    if L.gnx_device_count() <= 0:
        # no CPU fallback; the device is looked for after the argument checks
        with pytest.raises(_lib.GnxError) as ei:
            align.AffineGapLocalSpan(t, q, align.DefaultScoreMatrix, -400, -30)
        assert ei.value.code == _lib.GNX_EDEVICE
        with pytest.raises(_lib.GnxError) as ei:
            _lib.locate_span_batch_windows(local, t, [0], [len(t)], q, [0], [len(q)])
        assert ei.value.code == _lib.GNX_EDEVICE


# ---- the inputs of the lemma and of the model -------------------------------------------------------------------------------------
def _related(rng, tlen, alphabet):
    """A mutated read from inside a target of tlen bases; the read starts in the target's right two thirds."""
    t = rng.integers(0, alphabet, size=tlen).astype(np.uint8)
    m = int(rng.integers(40, 180))
    o = int(rng.integers(tlen // 3, tlen - m))
    return t, common.mutate(rng, t[o:o + m], sub=0.04, indel=0.02, geo=0.4, alphabet=alphabet)


def _lemma_cases():
    """[(matrix name, gapOpen, gapExtend, targets, queries, related?)]: about 1 500 pairs."""
    rng = np.random.default_rng(419)
    cases = []
    pens = pyref_span.PENALTIES + [(-400, 0), (0, 0)]  # gapExtend == 0: no bound, lo = 0
    for name in pyref_span.all_matrices():
        for (go, ge) in pens:
            rel_t, rel_q = [], []
            if ge < 0:
                for _ in range(12):
                    t, q = _related(rng, int(rng.integers(2000, 3001)), 4)
                    rel_t.append(t)
                    rel_q.append(q)
                cases.append((name, go, ge, rel_t, rel_q, True))
            ts, qs = common.random_pairs(int(rng.integers(1 << 30)), 16, 1, 400, 1, 400)
            # two-letter sequences: ties at almost every cell
            for _ in range(12):
                ts.append(rng.integers(0, 2, size=int(rng.integers(1, 120))).astype(np.uint8))
                qs.append(rng.integers(0, 2, size=int(rng.integers(1, 90))).astype(np.uint8))
            cases.append((name, go, ge, ts, qs, False))
    return cases


@pytest.fixture(scope="module")
def lemma_cases():
    cases = _lemma_cases()
    mats = pyref_span.all_matrices()
    full = [pyref_span.spans_from_oracle(mats[name], go, ge, ts, qs) for name, go, ge, ts, qs, _ in cases]
    return cases, full


def test_lemma_window_reproduces_the_route_on_the_oracle(lemma_cases):
    cases, full = lemma_cases
    mats = pyref_span.all_matrices()
    n_pairs = n_related = related_pos = zero = 0
    for (name, go, ge, ts, qs, related), (S, start, end) in zip(cases, full):
        los = [pyref_span.window_lo(S[p], end[p], len(qs[p]), mats[name], go, ge) for p in range(len(ts))]
        wins = [ts[p][los[p]:int(end[p])] for p in range(len(ts))]
        wS, wstart, wend = pyref_span.spans_from_oracle(mats[name], go, ge, wins, qs)
        for p in range(len(ts)):
            what = (name, go, ge, p, len(ts[p]), len(qs[p]), los[p])
            assert 0 <= los[p] <= start[p] <= end[p] <= len(ts[p]), what
            assert int(wS[p]) == int(S[p]), what
            assert int(wstart[p]) == int(start[p]) - los[p], what
            assert int(wend[p]) == len(wins[p]), what  # no trailing ColD run
            if ge == 0:
                assert los[p] == 0, what
        n_pairs += len(ts)
        zero += sum(1 for x in los if x == 0)
        if related:
            n_related += len(ts)
            related_pos += sum(1 for x in los if x > 0)
    print("lemma: %d pairs, lo > 0 in %d of %d related pairs, lo == 0 in %d pairs" % (n_pairs, related_pos, n_related, zero))
    assert n_pairs >= 1400
    assert 2 * related_pos >= n_related and zero > 0


@pytest.mark.parametrize("strip", [192, 7])
def test_scalar_model_of_the_kernel_equals_the_oracle(lemma_cases, strip):
    """The recurrence as span_origin_kernel has it (pyref_span.model_span), on the lemma's inputs thinned to what a Python loop can
    do: of every case the first pairs whose window DP has at most 40 000 cells; queries of more than one strip are among them."""
    cases, full = lemma_cases
    mats = pyref_span.all_matrices()
    done = multi = 0
    for (name, go, ge, ts, qs, related), (S, start, end) in zip(cases, full):
        took = [0, 0]  # per case at most two pairs of one strip and two of several
        for p in range(len(ts)):
            m = len(qs[p])
            lo = pyref_span.window_lo(S[p], end[p], m, mats[name], go, ge)
            several = 1 if m > strip else 0
            if (int(end[p]) - lo) * m > 40000 or took[several] >= 2:
                continue
            got_start, got_score, got_lo = pyref_span.model_span(ts[p], qs[p], mats[name], go, ge, S[p], end[p], strip=strip)
            assert (got_score, got_start, got_lo) == (int(S[p]), int(start[p]), lo), (name, go, ge, p, len(ts[p]), m, strip)
            took[several] += 1
            done += 1
            multi += several
    print("model: %d pairs, %d of more than one strip of %d" % (done, multi, strip))
    assert done >= 100 and multi >= 20


# ---- the kernel's resources, from the gfx950 code object inside the built library -------------------------------------------------
def _kernel_notes(tmp_path):
    import __graft_entry__ as g
    g.build()
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", _lib.LIB_PATH])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        f = {k: v for k, v in re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + blk)}
        if "name" in f and ".kd" not in f["name"]:
            out[f["name"]] = {k: int(f[k]) for k in ("agpr_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return out


SPAN_PINS = {"span_origin_kernel": (101, 0)}  # (VGPRs, LDS bytes) as built


def test_span_kernel_resources(tmp_path):
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    notes = _kernel_notes(tmp_path)
    for name, (vgprs, lds) in SPAN_PINS.items():
        match = [k for n, k in notes.items() if name in n]
        assert len(match) == 1, (name, sorted(notes))
        k = match[0]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["agpr_count"] == 0, (name, k)
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k)
        # DESIGN 4.19 claims four waves per SIMD: at most 104 registers (512 per lane, granule 8), and LDS that lets 16 one-wave
        # workgroups share a CU's 160 KB
        assert 512 // ((k["vgpr_count"] + 7) // 8 * 8) == 4, (name, k)
        assert k["group_segment_fixed_size"] * 16 <= 160 * 1024, (name, k)
    span = [k for n, k in notes.items() if "cigar_target_span_kernel" in n]
    assert len(span) == 1 and span[0]["private_segment_fixed_size"] == 0 and span[0]["vgpr_spill_count"] == 0


def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_span_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    rc = subprocess.call([BIN])
    assert rc in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box
