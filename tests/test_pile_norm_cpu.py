"""Left-normalised alleles of the pile without a GPU: the restatement (tests/pyref_pile_norm.py) on the rule's hand pins and its properties
on random repeat references, symbols and keyword arguments, the C ABI's argument checks, the shared arithmetic of csrc/norm_shift.h as a
stand-alone program under the address and undefined-behaviour sanitizers, the C++ mirror's build, and the resources of the norm_* kernels."""
import ctypes
import os
import inspect
import subprocess

import numpy as np
import pytest

import pyref_pile_alleles as ref
import pyref_pile_norm as norm
from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIRROR_SRC = os.path.join(ROOT, "tests", "cpp", "pile_norm_mirror_test.cpp")
MIRROR_BIN = os.path.join(ROOT, "tests", "cpp", "pile_norm_mirror_test.bin")
SHIFT_SRC = os.path.join(ROOT, "tests", "cpp", "norm_shift_test.cpp")
NAMES = ("gnx_pileup_alleles_norm", "gnx_pileup_indel_calls_norm")
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _lib_built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _codes(text):
    return [int(b) for b in dna.StringToBases(text)]


# ---- 1. the pins of the rule (0-based): (reference, lo, kind, x, L or inserted bases) -> (x, L or inserted bases) ----
PINS = [
    ("GATTTTTC", 0, "del", 6, 1, 2, 1), ("GATTTTTC", 0, "del", 5, 2, 2, 2),
    ("GATTTTTC", 0, "ins", 6, "T", 1, "T"), ("GATTTTTC", 0, "ins", 6, "TT", 1, "TT"), ("GATTTTTC", 0, "ins", 6, "GT", 5, "TG"), ("GATTTTTC", 0, "ins", 6, "NT", 5, "TN"),
    ("GCACACAT", 0, "del", 5, 2, 1, 2), ("GCACACAT", 0, "ins", 6, "CA", 0, "CA"), ("GCACACAT", 0, "ins", 6, "ACA", 3, "ACA"),
    ("GCACACAT", 3, "del", 5, 2, 3, 2), ("GCACACAT", 3, "ins", 6, "CA", 3, "AC"),
    ("GATTNTTC", 0, "del", 6, 1, 5, 1),
    ("TTTTTTTC", 0, "del", 6, 1, 0, 1), ("TTTTTTTC", 0, "ins", 6, "T", 0, "T"),
]


@pytest.mark.parametrize("pin", PINS, ids=lambda p: "%s-lo%d-%s-%d-%s" % p[:5])
def test_pins(pin):
    text, lo, kind, x, what, want_x, want = pin
    R = _codes(text)
    if kind == "del":
        assert norm.shift_deletion(R, x, what, lo) == want_x and want == what
        assert norm.normalize(R, x, ref.DEL, what, lo) == (want_x, ref.DEL, what)
    else:
        assert norm.shift_insertion(R, x, _codes(what), lo) == (want_x, _codes(want))
        assert norm.normalize(R, x, ref.INS, ref.pack(_codes(what)), lo) == (want_x, ref.INS, ref.pack(_codes(want)))
    assert norm.normalize(R, x, ref.LONG_INS, 30, lo) == (x, ref.LONG_INS, 30)  # a long insertion stays


# ---- 2. properties on random repeat references ----
def _random_case(rng):
    period = int(rng.integers(1, 6))
    n = int(rng.integers(40, 200))
    R = [(k % period) % 4 if rng.integers(0, 19) else int(rng.integers(0, 5)) for k in range(n)]
    L = int(rng.integers(1, 24))
    x = int(rng.integers(1, n - L))
    lo = int(rng.integers(0, x + 1))
    s = [int(rng.integers(0, period)) % 4 if rng.integers(0, 9) else int(rng.integers(0, 5)) for _ in range(int(rng.integers(1, 22)))]
    return R, x, L, s, lo


def _apply(R, kind, x, what):
    """the haplotype: the allele applied to the reference"""
    return R[:x] + R[x + what:] if kind == "del" else R[:x + 1] + list(what) + R[x + 1:]


def test_properties_on_random_repeats():
    rng = np.random.default_rng(427)
    moved = clamped = stopped_by_n = 0
    for _ in range(4000):
        R, x, L, s, lo = _random_case(rng)
        # a deletion
        nx = norm.shift_deletion(R, x, L, lo)
        assert lo <= nx <= x and norm.shift_deletion(R, nx, L, lo) == nx                        # idempotent
        assert nx == lo or R[nx - 1] >= 4 or R[nx - 1] != R[nx + L - 1]                           # no further shift is possible
        assert all(R[y] < 4 and R[y] == R[y + L] for y in range(nx, x))                           # every step was one
        if all(b < 4 for b in R[nx:x + L]):
            assert _apply(R, "del", nx, L) == _apply(R, "del", x, L)                              # the haplotype is unchanged
        moved += nx < x
        clamped += nx == lo and lo > 0 and R[lo - 1] < 4 and R[lo - 1] == R[lo + L - 1]
        stopped_by_n += nx > lo and R[nx - 1] >= 4
        # an insertion
        ix, t = norm.shift_insertion(R, x, s, lo)
        assert lo <= ix <= x and len(t) == len(s) and norm.shift_insertion(R, ix, t, lo) == (ix, t)
        assert ix == lo or R[ix] >= 4 or t[-1] >= 4 or R[ix] != t[-1]
        assert sorted(t) == sorted(s) or ix <= x - len(s)                                         # a rotation while the shift is short
        if ix > x - len(s):
            d = x - ix
            assert t == (s[len(s) - d:] + s[:len(s) - d] if d else s)
        if all(b < 4 for b in R[ix:x + 1]) and all(b < 4 for b in s):
            assert _apply(R, "ins", ix, t) == _apply(R, "ins", x, s)
        moved += ix < x
    assert moved > 1000 and clamped > 20 and stopped_by_n > 20                                    # (conditions on the inputs)


def test_counts_are_preserved_under_merging():
    rng = np.random.default_rng(428)
    R = ([0, 1] + [3] * 30 + [2] + [0, 1, 2] * 12 + [3, 4] + [1] * 20 + [0]) * 2
    region = (3, len(R) - 10)
    alleles = ref.new_alleles()
    for _ in range(600):
        x = int(rng.integers(region[0], region[0] + region[1] - 30))
        kind = (ref.DEL, ref.INS, ref.LONG_INS)[int(rng.integers(0, 3))]
        key = int(rng.integers(1, 4)) if kind == ref.DEL else 22 + int(rng.integers(0, 3)) if kind == ref.LONG_INS else ref.pack([R[x]] * int(rng.integers(1, 4)) if rng.integers(0, 2) else [0, 1, 2])
        alleles.setdefault((x, kind, key), [0, 0])[int(rng.integers(0, 2))] += 1
    got = norm.normalized(alleles, R, region)
    assert len(got) < len(alleles) and all(region[0] <= p < region[0] + region[1] for p, _, _ in got)
    for kind in (ref.DEL, ref.INS, ref.LONG_INS):
        for s in (0, 1):
            assert sum(c[s] for (_, k, _), c in got.items() if k == kind) == sum(c[s] for (_, k, _), c in alleles.items() if k == kind) > 0
    assert {k: v for k, v in got.items() if k[1] == ref.LONG_INS} == {k: v for k, v in alleles.items() if k[1] == ref.LONG_INS}
    assert norm.normalized(got, R, region) == got
    # one allele seen at five units is one allele
    five = {(2 + k, ref.DEL, 1): [k, 1] for k in range(5)}
    assert norm.normalized(five, R, (0, len(R))) == {(2, ref.DEL, 1): [10, 5]}
    late = {(6 + k, ref.DEL, 1): [k, 1] for k in range(5)}
    assert norm.normalized(late, R, (4, len(R) - 4)) == {(4, ref.DEL, 1): [10, 5]}  # clamped at the region's start


# ---- 3. symbols, bindings, keyword arguments ----
def test_symbols_and_keywords():
    _lib_built()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in NAMES:
        assert hasattr(L, nm) and nm in _lib.EXPORTS
        assert getattr(_lib.lib(), nm).restype is ctypes.c_int and len(getattr(_lib.lib(), nm).argtypes) == (2 if nm.endswith("alleles_norm") else 3)
    for fn in (align.PileupAlleles, align.PileupIndelCalls, _lib.pileup_alleles, _lib.pileup_indel_calls):
        assert inspect.signature(fn).parameters["normalize"].default is False
    header = open(os.path.join(ROOT, "include", "gnx_align.h")).read()
    for nm in NAMES:
        assert "int %s(" % nm in header


# ---- 4. argument checks need no device ----
def _opts(min_depth=1, min_alt=1, num=1, den=2, both=0):
    return _lib.GnxPileCallOpts(min_depth, min_alt, num, den, both, 0)


def _calls_rc(o, give_calls=True, give_n=True):
    calls, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    rc = _lib.lib().gnx_pileup_indel_calls_norm(ctypes.byref(o) if o is not None else None, ctypes.byref(calls) if give_calls else None, ctypes.byref(n) if give_n else None)
    assert calls.value == SENTINEL and n.value == SENTINEL  # nothing was written
    return rc


def test_null_pointers_and_no_pile():
    L = _lib.lib()
    _lib.check(L.gnx_pileup_close())
    assert _calls_rc(None) == _lib.GNX_EINVAL
    assert _calls_rc(_opts(), give_calls=False) == _lib.GNX_EINVAL
    assert _calls_rc(_opts(), give_n=False) == _lib.GNX_EINVAL
    assert _calls_rc(_opts(min_alt=0)) == _lib.GNX_EINVAL and b"gnx_pile_call_opts" in L.gnx_last_error()
    assert _calls_rc(_opts()) == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    out, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    assert L.gnx_pileup_alleles_norm(None, ctypes.byref(n)) == _lib.GNX_EINVAL and L.gnx_pileup_alleles_norm(ctypes.byref(out), None) == _lib.GNX_EINVAL
    assert L.gnx_pileup_alleles_norm(ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    assert out.value == SENTINEL and n.value == SENTINEL
    for call in (lambda: align.PileupAlleles(normalize=True), lambda: align.PileupIndelCalls(1, 1, normalize=True)):
        with pytest.raises(_lib.GnxError) as ei:
            call()
        assert ei.value.code == _lib.GNX_EINVAL


# ---- 5. csrc/norm_shift.h as a program of its own, under the sanitizers ----
def test_norm_shift_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "norm_shift_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "gonomics_amd", "csrc"), "-o", exe, SHIFT_SRC])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "norm_shift_test ok" in res.stdout, res.stdout + res.stderr


# ---- 6. the C++ mirror ----
def _build_cpp():
    _lib_built()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", MIRROR_BIN, MIRROR_SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_pile_norm_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    assert subprocess.call([MIRROR_BIN]) in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


# ---- 7. kernel resources, from the gfx950 code object inside the built library ----
# name -> (VGPRs, LDS bytes) as built
NORM_PINS = {"norm_shift_kernel": (74, 0)}


def test_norm_kernel_resources(tmp_path):
    import test_kernel_resources as tkr
    if not os.path.exists(f"{tkr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kernels = tkr._kernels(tmp_path)
    mine = {n: k for n, k in kernels.items() if n.startswith("norm_")}
    assert sorted(mine) == sorted(NORM_PINS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)   # no scratch, no spills
        assert k["agpr_count"] == 0, (name, k)
        assert tkr._waves_per_simd(k) >= 4, (name, k["vgpr_count"])
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == NORM_PINS[name], (name, k)
