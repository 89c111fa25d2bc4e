"""gnx_pileup_alleles_norm / gnx_pileup_indel_calls_norm on the device against the literal restatement (tests/pyref_pile_norm.py): shifts
at the seams of norm_shift_kernel's chunks and of its wave steps at every dword phase, what stops a shift, merging, the call the feature
exists for, many long events in one launch, the life cycle, reports end to end into VCF text, the C++ mirror.  Every expectation is the
restatement's; the asserts beside it are conditions on the inputs."""
import ctypes
import functools
import io
import subprocess

import numpy as np
import pytest

import pile_allele_cases as pac
import pileup_cases as pc
import pyref_pile_alleles as ref
import pyref_pile_norm as norm
import summary_cases as sc
import test_pile_alleles_gpu as tag
import test_pileup_gpu as tpg
import test_summary_gpu as tsg
from gonomics_amd import _lib, align, vcf

pytestmark = pytest.mark.gpu

M, I, D = pc.M, pc.I, pc.D
_params, _add, _as_rows = tpg._params, tpg._add, tpg._as_rows
_allele_tuples, _call_tuples, _open_tracking = tag._allele_tuples, tag._call_tuples, tag._open_tracking
SHIFTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2079, 2080, 2081, 5003)
FLANK = 20


class Genome:
    """a reference grown repeat by repeat: plant() appends filler, then a unit repeated so that a deletion of one unit at x shifts by
    exactly `shift` (the base before the repeat breaks the period), with x at a chosen dword phase"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.g = []

    def filler(self, n):
        self.g += [int(b) for b in self.rng.integers(0, 4, size=n)]

    def plant(self, period, shift, phase=None, first=False):
        unit = [int(b) for b in self.rng.integers(0, 4, size=period)]
        if period > 1 and len(set(unit)) == 1:
            unit[-1] = (unit[0] + 1) % 4
        if not first:
            self.filler(FLANK + 8)
            while phase is not None and (len(self.g) + shift) % 16 != phase:
                self.filler(1)
        start = len(self.g)
        self.g += [unit[k % period] for k in range(shift + period)]
        x = start + shift
        if start > 0:
            self.g[start - 1] = (self.g[start - 1 + period] + 1) % 4
        self.g.append((self.g[len(self.g) - period] + 1) % 4)  # ... and nothing goes on behind it
        self.filler(FLANK + 8)
        return x, unit


class Batch:
    def __init__(self):
        self.windows, self.reads, self.strands, self.routes = [], [], [], []

    def deletion(self, g, x, L, strand=0, copies=1):
        route = [(FLANK, M), (L, D), (FLANK, M)]
        start = x - FLANK
        assert start >= 0 and start + 2 * FLANK + L <= len(g), (x, L)
        self._put(start, 2 * FLANK + L, pac.exact_read(g[start:start + 2 * FLANK + L], route), strand, route, copies)

    def insertion(self, g, behind, s, strand=0, copies=1):
        route = [(FLANK, M), (len(s), I), (FLANK, M)]
        start = behind - FLANK + 1
        assert start >= 0 and start + 2 * FLANK <= len(g), behind
        read = pac.exact_read(g[start:start + 2 * FLANK], route)
        read[FLANK:FLANK + len(s)] = s
        self._put(start, 2 * FLANK, read, strand, route, copies)

    def plain(self, g, start, n, strand=0, copies=1):
        self._put(start, n, np.array(g[start:start + n], dtype=np.uint8), strand, [(n, M)], copies)

    def _put(self, start, n, read, strand, route, copies):
        for _ in range(copies):
            self.windows.append((start, n))
            self.reads.append(read)
            self.strands.append(strand)
            self.routes.append(route)

    def all(self):
        return self.windows, self.reads, self.strands, self.routes

    def part(self, lo, hi):
        return tuple(x[lo:hi] for x in self.all())


def _restated(g, region, batch, opts):
    """-> (plain alleles listed, normalised alleles listed, plain calls, normalised calls) of the restatement"""
    pile, alleles = pac.restate(g, region, *batch)
    moved = norm.normalized(alleles, g.tolist(), region)
    codes = g[region[0]:region[0] + region[1]]
    return ref.listed(alleles), ref.listed(moved), ref.calls(alleles, pile, codes, opts, region_start=region[0]), ref.calls(moved, pile, codes, opts, region_start=region[0])


def _calls(opts, normalize):
    return _call_tuples(_lib.pileup_indel_calls(opts["min_depth"], opts["min_alt"], opts["frac_num"], opts["frac_den"], opts["both_strands"], normalize=normalize))


def _both_coop(monkeypatch, check):
    for coop in (None, "0", "1"):
        if coop is None:
            monkeypatch.delenv("GNX_NORM_COOP", raising=False)
        else:
            monkeypatch.setenv("GNX_NORM_COOP", coop)
        check(coop)
    monkeypatch.delenv("GNX_NORM_COOP", raising=False)


@pytest.fixture
def reference(gpu_lib):
    def use(g):
        gpu_lib.set_reference(np.asarray(g, dtype=np.uint8))
    try:
        yield use
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 1. seams: planted shifts, every dword phase, every length ----
@functools.lru_cache(maxsize=None)
def _seam_case():
    G = Genome(431)
    b = Batch()
    planted = []  # (x, period, shift): a deletion of `period` at x shifts by `shift`; the unit inserted behind x + period - 1 by shift + period
    periods = (1, 2, 3, 7, 21)
    x0, _ = G.plant(7, 40, first=True)  # a repeat that reaches reference position 0
    planted.append((x0, 7, 40))
    for k, shift in enumerate(SHIFTS):
        planted.append(G.plant(periods[k % 5], shift)[:1] + (periods[k % 5], shift))
        if shift < 100:
            planted.append(G.plant(periods[(k + 2) % 5], shift)[:1] + (periods[(k + 2) % 5], shift))
    for phase in range(16):
        planted.append(G.plant((1, 3, 2, 7)[phase % 4], 33 + phase % 3, phase=phase)[:1] + ((1, 3, 2, 7)[phase % 4], 33 + phase % 3))
    for L in (15, 16, 17, 33, 100):
        planted.append(G.plant(L, 40)[:1] + (L, 40))
    ins_plants = []
    for L in (1, 2, 20, 21):
        for shift in (0, 1, L + 3):
            ins_plants.append(G.plant(L, shift)[:1] + (L, shift))
    g = np.array(G.g, dtype=np.uint8)
    for k, (x, period, shift) in enumerate(planted):
        b.deletion(g, x, period, strand=k % 2)
        if period <= 21:
            b.insertion(g, x + period - 1, g[x:x + period], strand=(k + 1) % 2)
    ins_want = []
    for k, (x, L, shift) in enumerate(ins_plants):
        unit = g[x:x + L].copy()
        q = x + L - 1
        b.insertion(g, q, unit, strand=k % 2)  # d = shift + L: d == L where the repeat holds one unit, d > L beyond
        ins_want.append((q, unit, shift + L))
        if L > 1:
            for d in sorted({1, L // 2, L - 1}):  # d < L: a foreign base d bases from the end of the inserted unit
                s = unit.copy()
                s[L - 1 - d] = (s[L - 1 - d] + 1) % 4
                b.insertion(g, q, s, strand=(k + d) % 2)
                ins_want.append((q, s, d))
    b.insertion(g, planted[3][0] + planted[3][1] - 1, np.full(22, g[planted[3][0]], dtype=np.uint8))  # kind 3: stays
    return g, b, planted, ins_want


def test_seams(gpu_lib, reference, monkeypatch):
    g, b, planted, ins_want = _seam_case()
    # conditions on the inputs: the restatement's loops give exactly the planted shifts, at every dword phase; the insertions wrap
    assert {s for _, _, s in planted} >= set(SHIFTS) and {x % 16 for x, _, s in planted if s >= 33} == set(range(16))
    assert {p for _, p, _ in planted} >= {1, 2, 3, 7, 21, 15, 16, 17, 33, 100}
    for x, period, shift in planted:
        assert norm.shift_deletion(g, x, period, 0) == x - shift, (x, period, shift)
        if period <= 21:
            assert norm.shift_insertion(g, x + period - 1, list(g[x:x + period]), 0)[0] == max(x - shift - 1, 0)
    assert planted[0][0] - planted[0][2] == 0
    for q, s, d in ins_want:
        nx, t = norm.shift_insertion(g, q, list(s), 0)
        assert q - nx == d and t == [int(v) for v in np.roll(s, d)], (q, d)
    assert {(len(s), (d > len(s)) - (d < len(s))) for _, s, d in ins_want} >= {(L, c) for L in (2, 20, 21) for c in (-1, 0, 1)} | {(1, 0), (1, 1)}
    reference(g)
    p = _params()
    opts = pc.opts()
    lo = next(x for x, _, s in planted if s == 5003) - 1000  # inside the repeat of the longest shift
    for region in ((0, len(g)), (lo, len(g) - lo)):
        plain, moved, plain_calls, moved_calls = _restated(g, region, b.all(), opts)
        assert len(moved) <= len(plain) and moved != plain and (region[0] > 0 or any(w[1] == ref.LONG_INS for w in moved))
        assert region[0] == 0 or any(w[0] == lo for w in moved)  # clamped at the region's start

        def check(coop):
            _open_tracking(*region)
            _add(p, b.all())
            assert _allele_tuples(_lib.pileup_alleles()) == plain, coop
            assert _allele_tuples(_lib.pileup_alleles(normalize=True)) == moved, coop
            t = _lib.get_timing()
            assert t["fast_path"] == 18 and t["cells"] == align.PileupAlleleInfo()["events"] and 0 < t["dominant_ms"] < t["fill_ms"]
            assert _calls(opts, True) == moved_calls and _lib.get_timing()["fast_path"] == 19, coop
            assert _calls(opts, False) == plain_calls
            assert _allele_tuples(_lib.pileup_alleles()) == plain  # the log stays raw
        _both_coop(monkeypatch, check)
    assert len(moved_calls) > 0


# ---- 2. what stops a shift ----
def test_stops(gpu_lib, reference, monkeypatch):
    G = Genome(432)
    b = Batch()
    G.filler(30)
    while len(G.g) % 64 != 10:
        G.filler(1)
    spots = []
    for period, n_at in ((1, "edge_last"), (3, "edge_first"), (1, "inside"), (7, "inside"), (2, "none")):
        x, _ = G.plant(period, 300)
        spots.append((x, period, n_at))
    g = np.array(G.g, dtype=np.uint8)
    want_stop = {}
    for x, period, n_at in spots:
        inside = x - 150
        at = {"edge_last": inside | 63, "edge_first": (inside | 63) + 1, "inside": inside, "none": None}[n_at]
        if at is not None:
            g[at] = 4
            want_stop[x] = at
    for k, (x, period, n_at) in enumerate(spots):
        b.deletion(g, x, period, strand=k % 2)
        b.insertion(g, x + period - 1, g[x:x + period], strand=(k + 1) % 2)
    # a read N as the last and as an inner inserted base, in the clean repeat
    x, period, _ = spots[4]
    for where in (1, 0):
        s = np.array(g[x:x + 2], dtype=np.uint8)
        s[where] = 4
        b.insertion(g, x + 1, s)
    # conditions on the inputs
    for x, period, n_at in spots:
        nx = norm.shift_deletion(g, x, period, 0)
        if n_at == "none":
            assert nx == x - 300
        else:
            assert want_stop[x] < nx <= want_stop[x] + period and (period > 1 or nx == want_stop[x] + 1), (x, period, nx)
    assert want_stop[spots[0][0]] % 64 == 63 and want_stop[spots[1][0]] % 64 == 0
    assert norm.shift_insertion(g, x + 1, [int(g[x]), 4], 0) == (x + 1, [int(g[x]), 4])
    assert norm.shift_insertion(g, x + 1, [4, int(g[x + 1])], 0) == (x, [int(g[x + 1]), 4])
    reference(g)
    p = _params()
    opts = pc.opts()
    lo = spots[4][0] - 100
    for region in ((0, len(g)), (lo, len(g) - lo)):
        plain, moved, plain_calls, moved_calls = _restated(g, region, b.all(), opts)
        assert region[0] == 0 or (lo, ref.DEL, 2) in {w[:3] for w in moved}

        def check(coop):
            _open_tracking(*region)
            _add(p, b.all())
            assert _allele_tuples(_lib.pileup_alleles(normalize=True)) == moved, coop
            assert _calls(opts, True) == moved_calls and _calls(opts, False) == plain_calls, coop
        _both_coop(monkeypatch, check)


# ---- 3. merging, and the call the feature exists for ----
def test_merging_and_the_rule(gpu_lib, reference):
    G = Genome(433)
    x, _ = G.plant(1, 30)
    y, _ = G.plant(3, 30)
    G.filler(40)
    g = np.array(G.g, dtype=np.uint8)
    b = Batch()
    for k in range(5):  # one deletion and one insertion, each at five units, on both strands
        b.deletion(g, x - 5 * k, 1, strand=k % 2)
        b.insertion(g, x - 5 * k, g[x:x + 1], strand=(k + 1) % 2)
    other = np.array([(g[x] + 2) % 4], dtype=np.uint8)  # (neither the repeat's base nor the base before it)
    b.insertion(g, x - 31, other, copies=2)  # unrelated, at the insertion's final position
    b.deletion(g, x - 30, 2, strand=1)      # ... and at the deletion's
    # the rule: a deletion of one unit at two units, two reads each, under four plain reads
    for k in (0, 4):
        b.deletion(g, y - 3 * k, 3, strand=0)
        b.deletion(g, y - 3 * k, 3, strand=1)
    b.plain(g, y - 60, 100, copies=2)
    b.plain(g, y - 60, 100, strand=1, copies=2)
    reference(g)
    region = (0, len(g))
    opts = pc.opts(min_alt=3, frac=(1, 3))
    plain, moved, plain_calls, moved_calls = _restated(g, region, b.all(), opts)
    by_key = {w[:3]: w[3:] for w in moved}
    assert by_key[(x - 30, ref.DEL, 1)] == (5, 3) and by_key[(x - 31, ref.INS, ref.pack(g[x:x + 1]))] == (5, 2)
    assert by_key[(x - 31, ref.INS, ref.pack(other))] == (2, 2) and by_key[(x - 30, ref.DEL, 2)] == (1, 0)
    assert by_key[(y - 30, ref.DEL, 3)] == (4, 2) and sum(1 for w in plain if w[1] == ref.DEL and w[2] == 3) == 2
    assert not any(w[1] == ref.DEL and w[2] == 3 for w in plain_calls) and [w[:4] for w in moved_calls if w[1] == ref.DEL and w[2] == 3] == [(y - 30, ref.DEL, 3, 4)]
    _open_tracking(*region)
    _add(_params(), b.all())
    assert _allele_tuples(_lib.pileup_alleles()) == plain and _allele_tuples(_lib.pileup_alleles(normalize=True)) == moved
    assert _calls(opts, False) == plain_calls and _calls(opts, True) == moved_calls
    for kind in (ref.DEL, ref.INS):
        assert sum(w[3] for w in plain if w[1] == kind) == sum(w[3] for w in moved if w[1] == kind)
        assert sum(w[4] for w in plain if w[1] == kind) == sum(w[4] for w in moved if w[1] == kind)
    public = align.PileupIndelCalls(opts["min_depth"], opts["min_alt"], frac=(1, 3), normalize=True)
    assert [(d["pos"], d["kind"], d["length"], d["count"]) for d in public if d["kind"] == "del" and d["length"] == 3] == [(y - 30, "del", 3, 4)]
    assert [d["pos"] for d in align.PileupAlleles(normalize=True)] == [w[0] for w in moved]


# ---- 4. many long events in one launch ----
def test_many_events(gpu_lib, reference, monkeypatch):
    G = Genome(434)
    x, _ = G.plant(7, 5003)
    z, _ = G.plant(1, 9)
    g = np.array(G.g, dtype=np.uint8)
    b = Batch()
    for k in range(150):  # every one a shift of more than a lane's own chunk; together more than two waves' worth
        b.deletion(g, x - 7 * 3 * k, 7, strand=k % 2)
    for k in range(53):
        b.deletion(g, z - k % 9, 1, strand=k % 2)
    assert len(b.windows) == 203 and len(b.windows) % 64 != 0 and x - 7 * 3 * 149 - (x - 5003) > 64
    b.plain(g, x - 5003 - FLANK, 60, copies=2)  # (depth at the normalised position)
    reference(g)
    region = (0, len(g))
    opts = pc.opts(min_alt=100)
    plain, moved, plain_calls, moved_calls = _restated(g, region, b.all(), opts)
    assert len(plain) == 159 and [w for w in moved] == [(x - 5003, ref.DEL, 7, 150, 75), (z - 9, ref.DEL, 1, 53, 27)]
    assert plain_calls == [] and len(moved_calls) == 1

    def check(coop):
        _open_tracking(*region)
        _add(_params(), b.all())
        assert align.PileupAlleleInfo()["events"] == 203
        assert _allele_tuples(_lib.pileup_alleles(normalize=True)) == moved, coop
        assert _calls(opts, True) == moved_calls and _calls(opts, False) == plain_calls
    _both_coop(monkeypatch, check)


# ---- 5. life cycle ----
def test_lifecycle(gpu_lib, reference):
    g, b, _, _ = _seam_case()
    reference(g)
    L = _lib.lib()
    p = _params()
    region = (0, len(g))
    opts = pc.opts()
    half = len(b.windows) // 2
    out, n = ctypes.c_void_p(), ctypes.c_int64(-1)
    o = _lib.GnxPileCallOpts(1, 1, 1, 2, 0, 0)
    # a pile that does not track
    align.PileupOpen(*region)
    _add(p, b.part(0, 4))
    assert L.gnx_pileup_alleles_norm(ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL and b"does not track" in L.gnx_last_error() and n.value == -1
    assert L.gnx_pileup_indel_calls_norm(ctypes.byref(o), ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL and n.value == -1
    # an empty tracking pile: no alleles, and a pointer all the same
    _open_tracking(*region)
    assert L.gnx_pileup_alleles_norm(ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_OK and n.value == 0 and out.value
    L.gnx_free(out)
    assert L.gnx_pileup_indel_calls_norm(ctypes.byref(o), ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_OK and n.value == 0 and out.value
    L.gnx_free(out)
    # plain, normalised, plain; then more reads
    _add(p, b.part(0, half))
    plain, moved, plain_calls, moved_calls = _restated(g, region, b.part(0, half), opts)
    first = _lib.pileup_alleles()
    rows, info, ainfo = align.PileupGet().tobytes(), align.PileupInfo(), align.PileupAlleleInfo()
    assert _allele_tuples(first) == plain and _allele_tuples(_lib.pileup_alleles(normalize=True)) == moved
    assert _lib.pileup_alleles().tobytes() == first.tobytes()
    assert _calls(opts, True) == moved_calls and _calls(opts, False) == plain_calls
    assert (align.PileupGet().tobytes(), align.PileupInfo(), align.PileupAlleleInfo()) == (rows, info, ainfo)
    _add(p, b.part(half, len(b.windows)))
    plain, moved, plain_calls, moved_calls = _restated(g, region, b.all(), opts)
    assert _allele_tuples(_lib.pileup_alleles(normalize=True)) == moved and _allele_tuples(_lib.pileup_alleles()) == plain
    assert _calls(opts, True) == moved_calls and _calls(opts, False) == plain_calls
    # a stricter rule, and both strands
    for other in (pc.opts(min_alt=2), pc.opts(both_strands=1, frac=(1, 4)), pc.opts(min_depth=3)):
        pile, alleles = pac.restate(g, region, *b.all())
        assert _calls(other, True) == ref.calls(norm.normalized(alleles, g.tolist(), region), pile, g, other), other


# ---- 6. end to end: reports -> tracking pile -> normalised calls -> VCF ----
def test_reports_into_one_leftmost_vcf_record(gpu_lib, reference):
    rng = np.random.default_rng(435)
    g = rng.integers(0, 4, size=6000).astype(np.uint8)
    at, run = 3000, 12
    g[at:at + run] = 0
    g[at - 1], g[at + run] = 2, 1
    sample = np.delete(g, at + 5)  # the homopolymer is one base short, wherever an aligner puts the gap
    reads = []
    for k in range(12):
        o = at - 120 + 9 * k
        r = sample[o:o + 150].copy()
        reads.append(tsg._rc(r) if k % 2 else r)
    reference(g)
    gpu_lib.reference_index_build(tsg.K, 1)
    p = gpu_lib.make_params(sc.LOCAL, align.DefaultScoreMatrix, -400, -30)
    report = align.MapReadsReport(p, reads, tags=True, **tsg.VOTE)
    _open_tracking(0, len(g))
    assert align.PileupAddReport(p, reads, report) == 12
    moved = align.PileupAlleles(normalize=True)
    assert [(d["pos"], d["kind"], d["length"], d["count"], d["count_fwd"]) for d in moved] == [(at, "del", 1, 12, 6)]
    assert all(at <= d["pos"] < at + run and d["kind"] == "del" for d in align.PileupAlleles())
    indels = align.PileupIndelCalls(1, 3, normalize=True)
    out = io.StringIO()
    assert vcf.WriteVcf(out, "chr", g, [], indels) == 1
    assert pac.parse_vcf(out.getvalue()) == [("chr", at, "GA", "G", {"DP": 12, "AO": 12, "AOF": 6})]


# ---- 7. the C++ mirror ----
def test_cpp_pile_norm_mirror_runs(gpu_lib):
    import test_pile_norm_cpu
    test_pile_norm_cpu._build_cpp()
    assert subprocess.call([test_pile_norm_cpu.MIRROR_BIN]) == 0
