"""gnx_pileup_* on the device against the literal restatement (tests/pyref_pileup.py): the whole table in both forms of the walk and
across sub-batch cuts on the seams of the kernel, the edges of the region, 64 workgroups on the same counters, accumulation and `use`,
errors that must leave the table as it was, the calls (order included), the life cycle, the reports end to end, the C++ mirror."""
import ctypes
import functools
import itertools
import subprocess

import numpy as np
import pytest

import pileup_cases as pc
import pyref_pileup as ref
import summary_cases as sc
import test_summary_gpu as tsg
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu

FORMS = [{}, {"GNX_PILE_FORM": "0"}, {"GNX_PILE_FORM": "1"}]
CUTS = [{}, {"GNX_PILE_SUB": "1"}, {"GNX_PILE_SUB": "3"}]
SWITCHES = [dict(f, **c) for f, c in itertools.product(FORMS, CUTS)]


def _under(monkeypatch, env, call):
    for k in ("GNX_PILE_FORM", "GNX_PILE_SUB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return call()


def _params(mode=sc.LOCAL):
    _, mx, go, ge = sc.SCORING[0]
    return _lib.make_params(mode, mx, go, ge)


def _as_rows(pile):
    """the restatement's pile as a PILE_DTYPE array"""
    out = np.zeros(len(pile), dtype=_lib.PILE_DTYPE)
    for k, r in enumerate(pile):
        out["base"][k] = r["base"]
        out["del"][k] = r["del"]
        out["ins"][k] = r["ins"]
    return out


def _differences(got, want, start):
    bad = [start + int(k) for k in np.nonzero(got != want)[0][:5]]
    return [(x, got[x - start].tolist(), want[x - start].tolist()) for x in bad]


def _add(p, batch, use=None):
    windows, reads, strands, routes = batch
    align.PileupAdd(p, reads, windows, strands, routes, use=use)


def _columns(routes):
    return sum(r for route in routes for r, _ in route)


@pytest.fixture
def genome(gpu_lib):
    g, _ = tsg._resident_cases()
    gpu_lib.set_reference(g)
    try:
        yield g
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 1. seams: the summary's hand-made CIGARs as windows of one reference, both strands, every form and cut ----
@functools.lru_cache(maxsize=None)
def _seams():
    g, _ = tsg._resident_cases()
    names, windows, reads, strands, routes = pc.seam_batch(g)
    region = (0, len(g))
    return names, (windows, reads, strands, routes), _as_rows(pc.restate(g, region, windows, reads, strands, routes))


def test_seams(gpu_lib, genome, monkeypatch):
    names, batch, want = _seams()
    assert any(s < 70 and s + n > 60 for s, n in batch[0]) and any(s < 4100 and s + n > 4090 for s, n in batch[0])  # (windows over both N runs)
    assert want["base"][:, :, 4].sum() > 0 and want["ins"].sum() > 0 and want["del"].sum() > 0 and want["base"][:, 1].sum() > 0
    assert (want["_reserved"] == 0).all()
    p = _params()
    for env in SWITCHES:
        align.PileupOpen(0, len(genome))
        _under(monkeypatch, env, lambda: _add(p, batch))
        got = align.PileupGet()
        assert not _differences(got, want, 0), (env, _differences(got, want, 0))
        t = _lib.get_timing()
        assert t["fast_path"] == 14 and t["cells"] == _columns(batch[3])
        assert align.PileupInfo() == {"start": 0, "len": len(genome), "reads_added": len(names), "device_bytes": 56 * len(genome)}
    # one pair alone, a slice of the rows, and the empty batch
    align.PileupOpen(0, len(genome))
    one = tuple(x[:1] for x in batch)
    _add(p, one)
    align.PileupAdd(p, [], [], [], [])
    cat, off = _lib._cat([])
    _lib.pileup_add_by_offset(p, cat, off, [], [], [], np.zeros(0, _lib.CIGAR_DTYPE), np.zeros(1, np.int64))
    g, _ = tsg._resident_cases()
    alone = _as_rows(pc.restate(g, (0, len(g)), *one))
    s, n = one[0][0]
    assert (align.PileupGet(s, n) == alone[s:s + n]).all() and (align.PileupGet() == alone).all() and align.PileupInfo()["reads_added"] == 1
    assert align.PileupGet(5, 0).shape[0] == 0


def test_worked_values(gpu_lib):
    from gonomics_amd import dna
    g = np.zeros(300, np.uint8)
    g[pc.ALPHA_AT:pc.ALPHA_AT + 10] = dna.StringToBases(pc.ALPHA)
    gpu_lib.set_reference(g)
    try:
        for region in ((0, 300), (104, 3), (109, 40)):
            for strand, (read, route, where) in itertools.product((0, 1), pc.WORKED):
                align.PileupOpen(*region)
                align.PileupAdd(_params(), [dna.StringToBases(read)], [(pc.ALPHA_AT, 10)], [strand], [[align.Cigar(*c) for c in route]])
                assert (align.PileupGet() == _as_rows(pc.worked_pile(where, strand, region))).all(), (region, strand, read)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 2. the edges of the region ----
def test_region_edges(gpu_lib, genome, monkeypatch):
    batch = pc.edge_batch(genome)
    lo, n = pc.EDGE_REGION
    whole = _as_rows(pc.restate(genome, (0, len(genome)), *batch))
    want = _as_rows(pc.restate(genome, pc.EDGE_REGION, *batch))
    # conditions on the inputs: counts on both sides of either edge, D runs across both, I runs behind 39 / 40 / 4199 / 4200
    assert (want == whole[lo:lo + n]).all()
    for x in (lo - 1, lo, lo + n - 1, lo + n):
        assert whole["base"][x].sum() > 0 and whole["del"][x].sum() > 0 and whole["ins"][x].sum() > 0, x
    assert whole["base"][:lo].sum() > 0 and whole["base"][lo + n:].sum() > 0
    p = _params()
    for env in FORMS + CUTS[1:]:
        align.PileupOpen(lo, n)
        _under(monkeypatch, env, lambda: _add(p, batch))
        got = align.PileupGet()
        assert got.shape[0] == n and not _differences(got, want, lo), (env, _differences(got, want, lo))
    assert align.PileupInfo()["reads_added"] == len(batch[0])  # (a read wholly outside is added all the same: it is not an error)


# ---- 3. contention: 64 workgroups on the same counters ----
def test_contention(gpu_lib, genome, monkeypatch):
    batch = pc.contention_batch(genome)
    want = _as_rows(pc.restate(genome, (0, len(genome)), *tuple(x[:1] for x in batch)))
    assert want["del"].sum() == 1 and want["ins"].sum() == 1 and want["base"].sum() == 148
    p = _params()
    for env in FORMS:
        align.PileupOpen(0, len(genome))
        _under(monkeypatch, env, lambda: _add(p, batch))
        got = align.PileupGet()
        for f in ("base", "del", "ins"):
            assert (got[f] == 256 * want[f]).all(), (env, f)
        assert set(np.unique(got["base"])) == {0, 256} and align.PileupInfo()["reads_added"] == 256


# ---- 4. accumulation, `use`, and errors that leave the table as it was ----
def test_accumulation_and_use(gpu_lib, genome):
    names, batch, want = _seams()
    half = len(names) // 2
    p = _params()
    align.PileupOpen(0, len(genome))
    _add(p, tuple(x[:half] for x in batch))
    _add(p, tuple(x[half:] for x in batch))
    assert (align.PileupGet() == want).all() and align.PileupInfo()["reads_added"] == len(names)
    # use: all zeros changes nothing; a mask adds what the restatement adds for the chosen pairs
    _add(p, batch, use=[0] * len(names))
    assert (align.PileupGet() == want).all() and align.PileupInfo()["reads_added"] == len(names)
    assert _lib.get_timing()["cells"] == 0
    mask = [1 if k % 3 == 0 else 0 for k in range(len(names))]
    align.PileupOpen(0, len(genome))
    _add(p, batch, use=mask)
    chosen = tuple([v for v, m in zip(x, mask) if m] for x in batch)
    assert (align.PileupGet() == _as_rows(pc.restate(genome, (0, len(genome)), *chosen))).all()
    assert align.PileupInfo()["reads_added"] == sum(mask) and _lib.get_timing()["cells"] == _columns(chosen[3])


@pytest.mark.parametrize("what,code", [("op3", _lib.GNX_EINVAL), ("too_much_alpha", _lib.GNX_EINVAL), ("byte5_in_a_read", _lib.GNX_EBASE), ("strand_byte_2", _lib.GNX_EINVAL),
                                       ("global_mode", _lib.GNX_EINVAL), ("window_past_the_reference", _lib.GNX_EINVAL)])
def test_errors_leave_the_table_as_it_was(gpu_lib, genome, what, code):
    names, batch, _ = _seams()
    p = _params()
    align.PileupOpen(0, len(genome))
    _add(p, tuple(x[:6] for x in batch))
    before, info = align.PileupGet().tobytes(), align.PileupInfo()
    windows, reads, strands, routes = (list(x[:6]) for x in batch)
    last = len(windows)
    # a good pair first and a broken one behind it: nothing of the call may land
    windows.append((500, 20))
    reads.append(np.array(genome[500:520]))
    strands.append(0)
    routes.append([(20, sc.M)])
    if what == "op3":
        routes[last] = [(10, sc.M), (2, 3), (8, sc.M)]
    elif what == "too_much_alpha":
        routes[last] = [(15, sc.M), (6, sc.D), (5, sc.M)]
    elif what == "byte5_in_a_read":
        reads[last][7] = 5
    elif what == "strand_byte_2":
        strands[last] = 2
    elif what == "window_past_the_reference":
        windows[last] = (len(genome) - 10, 20)
    with pytest.raises((_lib.GnxError, IndexError)) as ei:
        align.PileupAdd(_params(_lib.GNX_AFFINE_GAP_HIGHMEM) if what == "global_mode" else p, reads, windows, strands, routes)
    assert (ei.value.__cause__.code if isinstance(ei.value, IndexError) else ei.value.code) == code
    assert align.PileupGet().tobytes() == before and align.PileupInfo() == info


# ---- 5. calls ----
def _call_tuples(calls):
    return [(int(c["pos"]), int(c["depth"]), int(c["count"]), int(c["count_fwd"]), int(c["kind"]), int(c["ref"]), int(c["alt"])) for c in calls]


def test_calls(gpu_lib, genome):
    batch = pc.call_batch(genome)
    start, n = pc.CALL_REGION
    pile = pc.restate(genome, pc.CALL_REGION, *batch)
    p = _params()
    align.PileupOpen(start, n)
    _add(p, batch)
    assert (align.PileupGet() == _as_rows(pile)).all()
    o = pc.CALL_OPTS
    want = ref.calls(pile, genome[start:start + n], o, region_start=start)
    # conditions on the inputs: every kind, a position with both a primary and an insertion call, thresholds met with equality, disagreement
    # inside both N runs that stays silent
    assert {w[4] for w in want} == {ref.SUB, ref.DEL, ref.INS}
    assert [w[4] for w in want if w[0] == 281] == [ref.SUB, ref.INS] and [(w[1], w[2]) for w in want if w[0] in (250, 251, 281)] == [(12, 8)] * 4
    assert 8 * o["frac_den"] == o["frac_num"] * 12
    for x in (65, 4095):
        assert genome[x] == 4 and sum(pile[x - start]["base"][0][:4]) > 0 and not any(w[0] == x for w in want)
    got = _lib.pileup_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"])
    assert _call_tuples(got) == want and (got["_pad"] == 0).all()
    t = _lib.get_timing()
    assert t["fast_path"] == 15 and t["cells"] == n
    # one read fewer than equality asks for; both strands; the public form; the empty result
    for opts in (pc.opts(min_alt=2, frac=(3, 4)), pc.opts(min_alt=2, frac=(2, 3), both_strands=1), pc.opts(min_depth=11, min_alt=9), pc.opts(frac=(1, 1 << 20)), pc.opts(frac=(1 << 20, 1 << 20))):
        got = _lib.pileup_calls(opts["min_depth"], opts["min_alt"], opts["frac_num"], opts["frac_den"], opts["both_strands"])
        assert _call_tuples(got) == ref.calls(pile, genome[start:start + n], opts, region_start=start), opts
    assert not any(w[0] in (250, 251, 281) for w in ref.calls(pile, genome[start:start + n], pc.opts(min_alt=2, frac=(3, 4)), region_start=start))
    public = align.PileupCalls(o["min_depth"], o["min_alt"], frac=(o["frac_num"], o["frac_den"]))
    assert [(d["pos"], d["depth"], d["count"], d["count_fwd"], ("sub", "del", "ins").index(d["kind"]), d["ref"], 0xFF if d["alt"] is None else d["alt"]) for d in public] == want
    calls_p, out_n = ctypes.c_void_p(), ctypes.c_int64(-1)
    oc = _lib.GnxPileCallOpts(1000, 1, 1, 2, 0, 0)
    assert _lib.lib().gnx_pileup_calls(ctypes.byref(oc), ctypes.byref(calls_p), ctypes.byref(out_n)) == _lib.GNX_OK and out_n.value == 0 and calls_p.value
    _lib.lib().gnx_free(calls_p)
    # a region that starts inside a tile's worth of positions and is no multiple of anything: the same calls, cut
    align.PileupOpen(37, 4100 - 37)
    _add(p, batch)
    cut = ref.calls(pc.restate(genome, (37, 4100 - 37), *batch), genome[37:4100], o, region_start=37)
    assert cut == [w for w in want if 37 <= w[0] < 4100] and _call_tuples(_lib.pileup_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], 0)) == cut


# ---- 6. life cycle ----
def test_lifecycle(gpu_lib, genome):
    L = _lib.lib()
    p = _params()
    batch = pc.contention_batch(genome, copies=3)
    align.PileupOpen(900, 400)
    _add(p, batch)
    assert align.PileupInfo() == {"start": 900, "len": 400, "reads_added": 3, "device_bytes": 400 * 56} and align.PileupGet()["base"].sum() == 3 * 148
    align.PileupOpen(1000, 64)  # open replaces: zeroed, another region
    assert align.PileupInfo() == {"start": 1000, "len": 64, "reads_added": 0, "device_bytes": 64 * 56} and not align.PileupGet().tobytes().strip(b"\0")
    rows = np.zeros(65, dtype=_lib.PILE_DTYPE)
    for first, count in ((0, 65), (64, 1), (-1, 1), (1, -1), (60, 5)):
        assert L.gnx_pileup_get(first, count, rows.ctypes.data) == _lib.GNX_EINVAL, (first, count)
    assert L.gnx_pileup_get(0, 64, None) == _lib.GNX_EINVAL and L.gnx_pileup_get(64, 0, None) == _lib.GNX_OK
    # a region that leaves the reference is refused and the open pile stays
    for start, n in ((len(genome), 1), (len(genome) - 5, 6), (0, len(genome) + 1), (-1, 5), (0, 0)):
        assert L.gnx_pileup_open(start, n) == _lib.GNX_EINVAL, (start, n)
    assert align.PileupInfo()["start"] == 1000
    align.PileupOpen(len(genome) - 1, 1)
    align.PileupOpen(0, len(genome))
    # the pile belongs to the reference: a new reference drops it, and so does the release
    _lib.set_reference(genome[:5000])
    assert L.gnx_pileup_info(None, None, None, None) == _lib.GNX_EINVAL
    with pytest.raises(_lib.GnxError) as ei:
        _add(p, batch)
    assert ei.value.code == _lib.GNX_EINVAL
    align.PileupOpen(0, 5000)
    _lib.set_reference(np.zeros(0, np.uint8))
    assert L.gnx_pileup_info(None, None, None, None) == _lib.GNX_EINVAL and L.gnx_pileup_open(0, 10) == _lib.GNX_EINVAL  # (no reference)
    _lib.set_reference(genome)
    align.PileupOpen(0, 100)
    align.PileupClose()
    align.PileupClose()
    assert L.gnx_pileup_info(None, None, None, None) == _lib.GNX_EINVAL


# ---- 7. end to end: reports -> pile -> calls ----
def test_reports_into_the_pile(gpu_lib):
    reads = tsg._simulated_reads()
    mx, go, ge = align.DefaultScoreMatrix, -400, -30
    gpu_lib.check(gpu_lib.lib().gnx_set_reference_synthetic(tsg.SYN_LEN, tsg.SYN_SEED))
    try:
        gpu_lib.reference_index_build(tsg.K, 1)
        p = gpu_lib.make_params(sc.LOCAL, mx, go, ge)
        report = align.MapReadsReport(p, reads, tags=True, **tsg.VOTE)
        syn = _lib.synthetic_reference_bases(0, tsg.SYN_LEN, tsg.SYN_SEED)
        region = (0, tsg.SYN_LEN)
        for min_mapq in (0, 30, 61):
            align.PileupOpen(*region)
            added = align.PileupAddReport(p, reads, report, min_mapq=min_mapq)
            pile = ref.new_pile(tsg.SYN_LEN)
            n = 0
            for rep, read in zip(report, reads):
                if rep["best"] >= 0 and rep["mapq"] >= min_mapq:
                    t_len = sum(r for r, o in rep["route"] if o != sc.I)
                    start = rep["window_start"]
                    ref.add(pile, sc.LOCAL, start, syn[start:start + t_len], tsg._rc(read) if rep["strand"] else read, rep["strand"], [tuple(c) for c in rep["route"]], region)
                    n += 1
            assert added == n == align.PileupInfo()["reads_added"]
            assert (align.PileupGet() == _as_rows(pile)).all(), min_mapq
            want = ref.calls(pile, syn, pc.opts())
            assert _call_tuples(_lib.pileup_calls(1, 1, 1, 2, 0)) == want, min_mapq
            if min_mapq == 0:  # (conditions on the inputs: both strands are there, and the reads do disagree with the reference somewhere)
                assert n > 50 and {ref.SUB, ref.DEL, ref.INS} <= {w[4] for w in want} and {rep["strand"] for rep in report if rep["best"] >= 0} == {0, 1}
            if min_mapq == 61:
                assert n == 0 and want == []
        # the index is rebuilt and the pile is still there; the pair report goes in the same way
        gpu_lib.reference_index_build(tsg.K, 1)
        assert align.PileupInfo()["len"] == tsg.SYN_LEN
        pairs = align.MapReadPairsReport(p, reads, 150, 600, 200, tags=True, **tsg.VOTE)
        align.PileupOpen(*region)
        assert align.PileupAddReport(p, reads, pairs) == sum(1 for d in pairs if d["best"] >= 0) == align.PileupInfo()["reads_added"]
        assert align.PileupAddReport(p, reads, []) == 0
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 8. the C++ mirror ----
def test_cpp_pileup_mirror_runs(gpu_lib):
    import test_pileup_cpu
    test_pileup_cpu._build_cpp()
    assert subprocess.call([test_pileup_cpu.BIN]) == 0
