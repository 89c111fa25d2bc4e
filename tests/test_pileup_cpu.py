"""The pile without a GPU: the restatement (tests/pyref_pileup.py) on the header's worked values and against the summary's counts, the
call rule pinned by hand, the C ABI's argument checks, the symbols and struct layouts, the C++ mirror's build, and the resources of the
pile_* kernels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
import pileup_cases as pc
import pyref_pileup as ref
import pyref_summary
import summary_cases as sc
from gonomics_amd import _lib, align, dna

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pileup_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "pileup_mirror_test.bin")
NAMES = ("gnx_pileup_open", "gnx_pileup_info", "gnx_pileup_add_by_offset", "gnx_pileup_get", "gnx_pileup_calls", "gnx_pileup_close")
SENTINEL = 0x5A5A5A5A5A5A5A5A


# ---- 1. the restatement: worked values ----
@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("region", [(100, 10), (0, 200), (104, 3), (90, 11), (109, 40), (110, 5)])
def test_pyref_on_the_worked_values(strand, region):
    alpha = dna.StringToBases(pc.ALPHA)
    for read, route, where in pc.WORKED:
        pile = ref.add(ref.new_pile(region[1]), pc.LOCAL, pc.ALPHA_AT, alpha, dna.StringToBases(read), strand, route, region)
        assert pile == pc.worked_pile(where, strand, region), (read, region)
        assert all(r["base"][1 - strand] == [0] * 5 and r["del"][1 - strand] == 0 and not any(r["ins"]) for r in pile)


# ---- 2. invariants against the summary's counts, region = the whole window ----
def _totals(alpha, beta, route, strand=0):
    n = len(alpha)
    pile = ref.add(ref.new_pile(max(n, 1)), pc.LOCAL, 0, alpha, beta, strand, route, (0, max(n, 1)))
    return (sum(sum(r["base"][strand]) for r in pile), sum(r["del"][strand] for r in pile), sum(r["ins"][strand] for r in pile))


def _check_invariants(alpha, beta, route, what):
    s, _ = pyref_summary.summarize(pc.LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150, alpha, beta, route)
    bases, dels, inss = _totals(alpha, beta, route)
    assert bases == s["n_equal"] + s["n_mismatch"], what
    assert dels == s["del_bases"], what
    assert inss <= s["gap_runs"], what
    return s, inss


def test_invariants_against_the_summary():
    for name, alpha, beta, route in sc.seam_cases():
        _check_invariants(alpha, beta, route, name)
    name, mx, go, ge = sc.SCORING[0]
    alphas, betas = sc.related_pairs(pc.LOCAL, 530, 200, 60)
    _, ops, off = oracle.align_batch(pc.LOCAL, mx, go, ge, alphas, betas, ci=10000, cj=10000, threads=4)
    counted = terminal = deleted = 0
    for k in range(len(alphas)):
        route = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])]
        s, inss = _check_invariants(alphas[k], betas[k], route, k)
        cols = pyref_summary.columns(route)
        i_runs = sum(1 for c, (a, b) in enumerate(zip([None] + cols, cols)) if b == pc.I and a != pc.I)
        counted += inss
        terminal += i_runs - inss
        deleted += s["del_bases"]
    # (conditions on the inputs: a counted insertion, a terminal one that is not counted, a deletion)
    assert counted > 0 and terminal > 0 and deleted > 0, (counted, terminal, deleted)


def test_terminal_insertions_count_nowhere():
    a = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.uint8)
    for route, want in [([(2, pc.I), (5, pc.M)], 0), ([(5, pc.M), (2, pc.I)], 0), ([(3, pc.D), (2, pc.I), (4, pc.M), (3, pc.D)], 0), ([(4, pc.M), (2, pc.I), (3, pc.D)], 0),
                        ([(2, pc.I), (3, pc.D), (4, pc.M)], 0), ([(2, pc.M), (1, pc.I), (0, pc.D), (2, pc.I), (2, pc.M)], 1), ([(2, pc.M), (1, pc.I), (1, pc.D), (2, pc.I), (2, pc.M)], 2),
                        ([(3, pc.D), (1, pc.M), (2, pc.I), (4, pc.M)], 1)]:
        m = sum(r for r, o in route if o != pc.D)
        assert _totals(a, np.zeros(m, np.uint8), route)[2] == want, route


# ---- 3. the call rule, pinned by hand ----
@pytest.mark.parametrize("pin", pc.CALL_PINS, ids=lambda p: p[0])
def test_call_rule_pins(pin):
    name, code, row, opts, want = pin
    # the pinned row between two empty ones, at position 1001 of a region that starts at 1000
    got = ref.calls([pc.row(), row, pc.row()], [0, code, 0], opts, region_start=1000)
    assert got == [(1001,) + w for w in want], name


def test_calls_are_ordered_by_position():
    rows = [pin[2] for pin in pc.CALL_PINS if pin[3] == pc.opts()]
    codes = [pin[1] for pin in pc.CALL_PINS if pin[3] == pc.opts()]
    got = ref.calls(rows, codes, pc.opts())
    assert [g[0] for g in got] == sorted(g[0] for g in got) and {g[4] for g in got} == {ref.SUB, ref.DEL, ref.INS}
    both = [g for g in got if [h[0] for h in got].count(g[0]) == 2]
    assert [g[4] for g in both] == [ref.SUB, ref.INS]


# ---- 4. symbols and layouts ----
def test_symbols_and_structs():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in NAMES:
        assert hasattr(L, nm) and nm in _lib.EXPORTS
    for nm in ("PileupOpen", "PileupAdd", "PileupGet", "PileupCalls", "PileupInfo", "PileupClose", "PileupAddReport"):
        assert callable(getattr(align, nm))
    assert _lib.PILE_DTYPE.itemsize == 64 and _lib.PILE_CALL_DTYPE.itemsize == 24 and ctypes.sizeof(_lib.GnxPileCallOpts) == 24
    assert [_lib.PILE_DTYPE.fields[f][1] for f in ("base", "del", "ins", "_reserved")] == [0, 40, 48, 56]


# ---- 5. argument checks need no device ----
def _opts(min_depth=1, min_alt=1, num=1, den=2, both=0):
    return _lib.GnxPileCallOpts(min_depth, min_alt, num, den, both, 0)


def _calls_rc(o, give_calls=True, give_n=True):
    calls, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    rc = _lib.lib().gnx_pileup_calls(ctypes.byref(o) if o is not None else None, ctypes.byref(calls) if give_calls else None, ctypes.byref(n) if give_n else None)
    assert calls.value == SENTINEL and n.value == SENTINEL  # nothing was written
    return rc


@pytest.mark.parametrize("bad", [dict(min_depth=0), dict(min_depth=-3), dict(min_alt=0), dict(num=0), dict(num=-1), dict(num=3, den=2), dict(den=(1 << 20) + 1, num=1),
                                 dict(den=0, num=0), dict(both=2), dict(both=-1)], ids=str)
def test_call_options_out_of_range(bad):
    _lib.check(_lib.lib().gnx_pileup_close())
    assert _calls_rc(_opts(**bad)) == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()


def test_call_null_pointers_and_no_pile():
    _lib.check(_lib.lib().gnx_pileup_close())
    assert _calls_rc(None) == _lib.GNX_EINVAL
    assert _calls_rc(_opts(), give_calls=False) == _lib.GNX_EINVAL
    assert _calls_rc(_opts(), give_n=False) == _lib.GNX_EINVAL
    assert _calls_rc(_opts(den=1 << 20, num=1 << 20)) == _lib.GNX_EINVAL  # in range: refused only because no pile is open
    assert b"no open pile" in _lib.lib().gnx_last_error()


class _Add:
    """one valid gnx_pileup_add_by_offset call of two pairs; a test breaks one thing"""

    def __init__(self):
        self.p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
        self.n = 2
        self.cat, self.off = _lib._cat([[0, 1, 2], [0, 1, 2, 3, 3]])
        self.start, self.len = np.array([0, 4], np.int64), np.array([4, 4], np.int64)
        self.strand, self.use = np.array([0, 1], np.uint8), np.array([1, 1], np.uint8)
        self.ops, self.ooff = align._routes_to_ops([[(3, 0), (1, 2)], [(1, 1), (4, 0)]])
        self.null = set()

    def ptr(self, name):
        return None if name in self.null else getattr(self, name).ctypes.data

    def run(self):
        return _lib.lib().gnx_pileup_add_by_offset(None if "p" in self.null else ctypes.byref(self.p), self.n, self.ptr("cat"), self.ptr("off"), self.ptr("start"), self.ptr("len"),
                                                  self.ptr("strand"), self.ptr("ops"), self.ptr("ooff"), self.ptr("use"))


def _b_null(name):
    return lambda c: c.null.add(name)


def _b_set(attr, index, value, field=None):
    def brk(c):
        (getattr(c, attr)[field] if field else getattr(c, attr))[index] = value
    return brk


ADD_BREAKS = {"null_p": _b_null("p"), "null_read_off": _b_null("off"), "null_ref_start": _b_null("start"), "null_ref_len": _b_null("len"), "null_strand": _b_null("strand"),
              "null_ops": _b_null("ops"), "null_ops_off": _b_null("ooff"), "null_reads": _b_null("cat"), "negative_count": lambda c: setattr(c, "n", -1),
              "mode_global": lambda c: setattr(c.p, "mode", _lib.GNX_AFFINE_GAP_HIGHMEM), "mode_unknown": lambda c: setattr(c.p, "mode", 5),
              "ops_off_start": _b_set("ooff", 0, 1), "ops_off_order": _b_set("ooff", 1, 5), "op3": _b_set("ops", 1, 3, "op"), "negative_run": _b_set("ops", 2, -1, "run_length"),
              "too_much_alpha": _b_set("ops", 1, 2, "run_length"), "too_much_beta": _b_set("ops", 2, 2, "run_length"), "window_start": _b_set("start", 0, -1),
              "window_len": _b_set("len", 1, -2), "strand_byte_2": _b_set("strand", 1, 2), "strand_byte_255": _b_set("strand", 0, 255)}


@pytest.mark.parametrize("what", sorted(ADD_BREAKS))
def test_add_argument_errors_need_no_device(what):
    _lib.check(_lib.lib().gnx_pileup_close())
    c = _Add()
    ADD_BREAKS[what](c)
    assert c.run() == _lib.GNX_EINVAL, _lib.lib().gnx_last_error()
    assert b"no open pile" not in _lib.lib().gnx_last_error()  # (refused for what was broken, not for the missing pile)


def test_entries_without_a_pile():
    L = _lib.lib()
    assert L.gnx_pileup_close() == _lib.GNX_OK and L.gnx_pileup_close() == _lib.GNX_OK
    c = _Add()
    assert c.run() == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    c.use = None
    c.null.add("use")
    assert c.run() == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    rows = np.full(16, SENTINEL, dtype=np.int64)
    assert L.gnx_pileup_get(0, 1, rows.ctypes.data) == _lib.GNX_EINVAL and (rows == SENTINEL).all()
    info = np.full(4, SENTINEL, dtype=np.int64)
    assert L.gnx_pileup_info(info.ctypes.data, info.ctypes.data + 8, info.ctypes.data + 16, info.ctypes.data + 24) == _lib.GNX_EINVAL and (info == SENTINEL).all()
    assert L.gnx_pileup_info(None, None, None, None) == _lib.GNX_EINVAL
    assert _calls_rc(_opts()) == _lib.GNX_EINVAL
    for call in (lambda: align.PileupGet(), lambda: align.PileupInfo(), lambda: align.PileupCalls(1, 1), lambda: align.PileupAdd(c.p, [[0]], [(0, 1)], [0], [[(1, 0)]])):
        with pytest.raises(_lib.GnxError) as ei:
            call()
        assert ei.value.code == _lib.GNX_EINVAL


def test_open_argument_errors_and_a_valid_call_without_a_device():
    """no CPU fallback: a valid gnx_pileup_open is GNX_EDEVICE without a device, after the argument checks (with one, and no resident
    reference in this process, it is GNX_EINVAL)"""
    L = _lib.lib()
    has_gpu = L.gnx_device_count() > 0
    for start, length in ((0, 0), (0, -1), (-1, 10), (5, -(1 << 40))):
        assert L.gnx_pileup_open(start, length) == _lib.GNX_EINVAL, (start, length)
    if not has_gpu:
        assert L.gnx_pileup_open(0, 10) == _lib.GNX_EDEVICE
        with pytest.raises(_lib.GnxError) as ei:
            align.PileupOpen(0, 10)
        assert ei.value.code == _lib.GNX_EDEVICE
    assert L.gnx_pileup_info(None, None, None, None) == _lib.GNX_EINVAL or has_gpu  # nothing was opened on the way


# ---- 6. the C++ mirror ----
def _build_cpp():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_pileup_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    assert subprocess.call([BIN]) in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box


# ---- 7. kernel resources, from the gfx950 code object inside the built library ----
# name -> (VGPRs, LDS bytes) as built
PILE_PINS = {"pile_add_kernel": (74, 0), "pile_call_kernel<false>": (80, 0), "pile_call_kernel<true>": (77, 0)}


def test_pile_kernel_resources(tmp_path):
    import test_kernel_resources as tkr
    if not os.path.exists(f"{tkr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kernels = tkr._kernels(tmp_path)
    mine = {n: k for n, k in kernels.items() if n.startswith("pile_")}
    assert sorted(mine) == sorted(PILE_PINS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)   # no scratch, no spills
        assert k["agpr_count"] == 0, (name, k)
        assert tkr._waves_per_simd(k) >= 4, (name, k["vgpr_count"])
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == PILE_PINS[name], (name, k)
