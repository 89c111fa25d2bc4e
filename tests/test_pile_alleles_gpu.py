"""gnx_pileup_track_alleles / gnx_pileup_alleles / gnx_pileup_indel_calls on the device against the literal restatement
(tests/pyref_pile_alleles.py): the seams of the maximal-run logic under every sub-batch cut, the edges of the region, 64 workgroups
appending to one log that has to grow, errors that must leave everything as it was, the life cycle, the indel calls (order included),
the reports end to end into VCF text, the C++ mirror."""
import ctypes
import functools
import io
import subprocess

import numpy as np
import pytest

import pile_allele_cases as pac
import pileup_cases as pc
import pyref_pile_alleles as ref
import pyref_pileup
import summary_cases as sc
import test_pileup_gpu as tpg
import test_summary_gpu as tsg
from gonomics_amd import _lib, align, vcf

pytestmark = pytest.mark.gpu

genome = tpg.genome  # (the fixture: the resident reference of tsg._resident_cases())
_params, _add, _under, _as_rows = tpg._params, tpg._add, tpg._under, tpg._as_rows


def _allele_tuples(got):
    """device alleles as the restatement lists them: (pos, kind, key, count, count_fwd); the fields the key does not cover are checked here"""
    out = []
    for a in got:
        kind, seq, length = int(a["kind"]), int(a["seq"]), int(a["length"])
        assert kind in (ref.DEL, ref.INS, ref.LONG_INS) and (a["_pad"] == 0).all()
        if kind == ref.INS:
            assert 1 <= length <= ref.SEQ_MAX and seq >> (3 * length) == 0 and all((seq >> (3 * k)) & 7 in (1, 2, 3, 4, 5) for k in range(length)), a
        else:
            assert seq == 0 and length >= 1 and (kind != ref.LONG_INS or length > ref.SEQ_MAX), a
        out.append((int(a["pos"]), kind, seq if kind == ref.INS else length, int(a["count"]), int(a["count_fwd"])))
    return out


def _call_tuples(got):
    assert (got["_pad"] == 0).all() and (got["_pad2"] == 0).all()
    return [t + (int(c["depth"]), int(c["ref"])) for t, c in zip(_allele_tuples(got), got)]


def _open_tracking(start, n, reserve=0):
    align.PileupOpen(start, n)
    align.PileupTrackAlleles(reserve)


# ---- 1. the seams of the maximal-run logic ----
@functools.lru_cache(maxsize=None)
def _seams():
    g, _ = tsg._resident_cases()
    names, windows, reads, strands, routes = pac.seam_batch(g)
    pile, alleles = pac.restate(g, (0, len(g)), windows, reads, strands, routes)
    return names, (windows, reads, strands, routes), _as_rows(pile), alleles


def test_seams(gpu_lib, genome, monkeypatch):
    names, batch, rows, alleles = _seams()
    want = ref.listed(alleles)
    routes = dict(zip(names, batch[3]))
    # conditions on the inputs: pieces on both sides of the block seam (runs 63 | 64), a run of 130 pieces, a block that begins with empty runs,
    # 21 and 22 inserted bases, an N among inserted bases, every allele from both strands, two deletions at one position, plans that record nothing
    for nm in ("d_over_the_block_seam/0", "i_over_the_block_seam/0"):
        assert routes[nm][63][1] == routes[nm][64][1] != sc.M and routes[nm][63][0] > 0 and routes[nm][64][0] > 0
    assert all(r == 0 for r, _ in routes["d_then_a_block_that_begins_empty/0"][64:73]) and routes["d_then_a_block_that_begins_empty/0"][73] == (3, sc.D)
    assert len(routes["d_130_pieces_over_two_seams/0"]) == 132
    by_key = {(p, k, key): (c, f) for p, k, key, c, f in want}
    assert all(c == 2 and f == 1 for c, f in by_key.values())
    assert (100 + 8 * 211 + 20, ref.DEL, 130) in by_key and (100 + 9 * 211 + 19, ref.LONG_INS, 130) in by_key
    assert {key for _, k, key in by_key if k == ref.LONG_INS} == {22, 130} and any(k == ref.INS and key.bit_length() in (61, 62, 63) for _, k, key in by_key)
    assert any(k == ref.INS and 5 in [(key >> (3 * d)) & 7 for d in range(21)] for _, k, key in by_key)
    assert sorted(key for p, k, key in by_key if p == pac.SHARED_START + 20 and k == ref.DEL) == [1, 7]
    silent = ("i_at_alpha_start", "i_first", "i_at_alpha_end", "i_last", "leading_and_trailing_d", "one_d_run", "one_d_run_in_pieces")
    g = np.asarray(genome)
    for nm, w, rd, st, rt in zip(names, *batch):
        assert (ref.events(w[0], rd, rt, (0, len(g))) == []) == (nm.split("/")[0] in silent), nm
    p = _params()
    for env in tpg.CUTS:
        _open_tracking(0, len(genome))
        _under(monkeypatch, env, lambda: _add(p, batch))
        t = _lib.get_timing()
        assert t["fast_path"] == 14 and t["cells"] == tpg._columns(batch[3]) and 0 < t["dominant_ms"] < t["fill_ms"]
        assert _allele_tuples(_lib.pileup_alleles()) == want, env
        t = _lib.get_timing()
        assert t["fast_path"] == 16 and t["cells"] == 2 * len(want)
        assert (align.PileupGet() == rows).all()
        assert align.PileupInfo() == {"start": 0, "len": len(genome), "reads_added": len(names), "device_bytes": 56 * len(genome)}
        info = align.PileupAlleleInfo()
        assert info["tracking"] and info["events"] == 2 * len(want) and info["device_bytes"] >= 16 * info["events"]
    # the public form
    public = align.PileupAlleles()
    assert [(d["pos"], ("del", "ins", "long_ins").index(d["kind"]) + 1, d["length"], d["count"], d["count_fwd"]) for d in public] == \
        [(w[0], w[1], w[2] if w[1] != ref.INS else (w[2].bit_length() + 2) // 3, w[3], w[4]) for w in want]
    assert all((d["seq"] is None) == (d["kind"] != "ins") and (d["seq"] is None or ref.pack(d["seq"]) == w[2]) for d, w in zip(public, want))


def test_worked_values(gpu_lib):
    from gonomics_amd import dna
    g = np.zeros(300, np.uint8)
    g[pc.ALPHA_AT:pc.ALPHA_AT + 10] = dna.StringToBases(pc.ALPHA)
    gpu_lib.set_reference(g)
    try:
        for region in ((0, 300), (103, 1), (106, 1), (104, 2), (107, 40)):
            for strand in (0, 1):
                for read, route, want in pac.WORKED:
                    _open_tracking(*region)
                    align.PileupAdd(_params(), [dna.StringToBases(read)], [(pc.ALPHA_AT, 10)], [strand], [[align.Cigar(*c) for c in route]])
                    inside = [w + (1, 1 - strand) for w in want if region[0] <= w[0] < region[0] + region[1]]
                    assert _allele_tuples(_lib.pileup_alleles()) == inside, (region, strand, read)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 2. the edges of the region ----
def test_region_edges(gpu_lib, genome, monkeypatch):
    batch = pac.edge_batch(genome)
    lo, n = pc.EDGE_REGION
    pile, alleles = pac.restate(genome, pc.EDGE_REGION, *batch)
    _, whole = pac.restate(genome, (0, len(genome)), *batch)
    want = ref.listed(alleles)
    # conditions on the inputs: both kinds at lo - 1, lo, lo + n - 1, lo + n; inside only the middle two; the deletion at lo - 1 reaches in and
    # bumps `del` there; the one at lo + n - 1 reaches out and keeps its whole length
    for x in (lo - 1, lo, lo + n - 1, lo + n):
        assert {k for p, k, _ in whole if p == x} == {ref.DEL, ref.INS}, x
    assert [(w[0], w[1], w[2]) for w in want if w[1] == ref.DEL] == [(lo, ref.DEL, 5), (lo + n - 1, ref.DEL, 5)]
    assert [w[0] for w in want if w[1] == ref.INS] == [lo, lo + n - 1] and len(want) == 4
    assert sum(pile[0]["del"]) == 2 and sum(pile[3]["del"]) == 2 and sum(pile[4]["del"]) == 1
    p = _params()
    for env in tpg.CUTS:
        _open_tracking(lo, n)
        _under(monkeypatch, env, lambda: _add(p, batch))
        assert _allele_tuples(_lib.pileup_alleles()) == want, env
        assert (align.PileupGet() == _as_rows(pile)).all()


# ---- 3. contention and growth ----
def test_contention_and_growth(gpu_lib, genome):
    batch = pc.contention_batch(genome)
    one = tuple(x[:1] for x in batch)
    _, alleles = pac.restate(genome, (0, len(genome)), *one)
    single = ref.listed(alleles)
    assert [(w[1], w[3]) for w in single] == [(ref.DEL, 1), (ref.INS, 1)]
    want = [(p, k, key, 256 * c, 256 * f) for p, k, key, c, f in single]
    p = _params()
    _open_tracking(0, len(genome))
    _add(p, batch)
    assert _allele_tuples(_lib.pileup_alleles()) == want and align.PileupAlleleInfo()["events"] == 512
    # a log of one event that has to grow, the batch in two halves, the query between the adds and twice behind them
    _open_tracking(0, len(genome), reserve=1)
    first_bytes = align.PileupAlleleInfo()["device_bytes"]
    assert first_bytes <= 64 and align.PileupAlleleInfo()["events"] == 0 and len(_lib.pileup_alleles()) == 0
    _add(p, tuple(x[:128] for x in batch))
    half_bytes = align.PileupAlleleInfo()["device_bytes"]
    assert _allele_tuples(_lib.pileup_alleles()) == [(q, k, key, 128 * c, 128 * f) for q, k, key, c, f in single]
    _add(p, tuple(x[128:] for x in batch))
    assert first_bytes < 256 * 16 <= half_bytes < 512 * 16 <= align.PileupAlleleInfo()["device_bytes"]
    assert _allele_tuples(_lib.pileup_alleles()) == want
    assert _allele_tuples(_lib.pileup_alleles()) == want and align.PileupAlleleInfo()["events"] == 512
    assert (align.PileupGet()["del"].sum(), align.PileupGet()["ins"].sum()) == (256, 256)
    # a `use` mask, on both strands
    names, sb, _, _ = _seams()
    mask = [1 if k % 3 == 0 else 0 for k in range(len(names))]
    chosen = tuple([v for v, m in zip(x, mask) if m] for x in sb)
    _open_tracking(0, len(genome))
    _add(p, sb, use=mask)
    assert _allele_tuples(_lib.pileup_alleles()) == ref.listed(pac.restate(genome, (0, len(genome)), *chosen)[1])
    events = align.PileupAlleleInfo()["events"]
    _add(p, sb, use=[0] * len(names))  # nobody is added: nothing is logged
    assert events > 0 and align.PileupAlleleInfo()["events"] == events
    assert _allele_tuples(_lib.pileup_alleles()) == ref.listed(pac.restate(genome, (0, len(genome)), *chosen)[1])


# ---- 4. errors leave everything as it was ----
@pytest.mark.parametrize("what,code", [("op3", _lib.GNX_EINVAL), ("too_much_alpha", _lib.GNX_EINVAL), ("byte5_in_a_read", _lib.GNX_EBASE), ("strand_byte_2", _lib.GNX_EINVAL),
                                       ("global_mode", _lib.GNX_EINVAL), ("window_past_the_reference", _lib.GNX_EINVAL)])
def test_errors_leave_everything_as_it_was(gpu_lib, genome, what, code):
    names, batch, _, _ = _seams()
    p = _params()
    _open_tracking(0, len(genome), reserve=1)
    _add(p, tuple(x[:6] for x in batch))
    before, info, ainfo, alleles = align.PileupGet().tobytes(), align.PileupInfo(), align.PileupAlleleInfo(), _lib.pileup_alleles().tobytes()
    assert ainfo["events"] > 0
    windows, reads, strands, routes = (list(x[:6]) for x in batch)
    reads = [np.array(r) for r in reads]
    last = len(windows)
    # a good pair with an indel first and a broken one behind it: nothing of the call may land, and the log may not even grow
    windows.append((500, 22))
    reads.append(np.array(genome[500:520]))
    strands.append(0)
    routes.append([(10, sc.M), (2, sc.D), (10, sc.M)])
    windows.append((600, 20))
    reads.append(np.array(genome[600:620]))
    strands.append(0)
    routes.append([(20, sc.M)])
    last += 1
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
    assert align.PileupGet().tobytes() == before and align.PileupInfo() == info and align.PileupAlleleInfo() == ainfo and _lib.pileup_alleles().tobytes() == alleles


# ---- 5. life cycle ----
def test_lifecycle(gpu_lib, genome):
    L = _lib.lib()
    p = _params()
    batch = pc.contention_batch(genome, copies=3)
    out, n = ctypes.c_void_p(), ctypes.c_int64(-1)
    o = _lib.GnxPileCallOpts(1, 1, 1, 2, 0, 0)
    # a pile that does not track: no alleles, and rows and calls as ever
    align.PileupOpen(900, 400)
    assert align.PileupAlleleInfo() == {"tracking": False, "events": 0, "device_bytes": 0}
    _add(p, batch)
    plain_rows, plain_calls, plain_info = align.PileupGet().tobytes(), _lib.pileup_calls(1, 1, 1, 2, 0).tobytes(), align.PileupInfo()
    assert L.gnx_pileup_alleles(ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL and b"does not track" in L.gnx_last_error() and n.value == -1
    assert L.gnx_pileup_indel_calls(ctypes.byref(o), ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL and n.value == -1
    # tracking after an add is refused, and the pile stays what it was
    assert L.gnx_pileup_track_alleles(0) == _lib.GNX_EINVAL and align.PileupAlleleInfo()["tracking"] is False
    assert L.gnx_pileup_track_alleles(-1) == _lib.GNX_EINVAL
    # the same batch on a tracking pile: the same rows, calls and info
    _open_tracking(900, 400)
    assert L.gnx_pileup_track_alleles(-1) == _lib.GNX_EINVAL and L.gnx_pileup_track_alleles(10) == _lib.GNX_OK  # (still empty: allowed again)
    _add(p, batch)
    assert align.PileupGet().tobytes() == plain_rows and _lib.pileup_calls(1, 1, 1, 2, 0).tobytes() == plain_calls and align.PileupInfo() == plain_info
    assert len(_lib.pileup_alleles()) == 2 and align.PileupAlleleInfo()["events"] == 6
    assert L.gnx_pileup_track_alleles(0) == _lib.GNX_EINVAL
    # open resets tracking
    align.PileupOpen(900, 400)
    assert align.PileupAlleleInfo() == {"tracking": False, "events": 0, "device_bytes": 0}
    assert L.gnx_pileup_alleles(ctypes.byref(out), ctypes.byref(n)) == _lib.GNX_EINVAL
    # a new reference drops the log with the pile; close does too
    _open_tracking(0, 100)
    _lib.set_reference(genome[:5000])
    assert L.gnx_pileup_allele_info(None, None, None) == _lib.GNX_EINVAL and L.gnx_pileup_track_alleles(0) == _lib.GNX_EINVAL
    _open_tracking(0, 5000)
    align.PileupClose()
    assert L.gnx_pileup_allele_info(None, None, None) == _lib.GNX_EINVAL
    align.PileupOpen(0, 5000)
    assert align.PileupAlleleInfo()["tracking"] is False
    _lib.set_reference(genome)


# ---- 6. indel calls ----
def test_indel_calls(gpu_lib, genome):
    batch = pac.call_batch(genome)
    start, n = pc.CALL_REGION
    pile, alleles = pac.restate(genome, pc.CALL_REGION, *batch)
    codes = genome[start:start + n]
    p = _params()
    _open_tracking(start, n)
    _add(p, batch)
    assert (align.PileupGet() == _as_rows(pile)).all() and _allele_tuples(_lib.pileup_alleles()) == ref.listed(alleles)
    o = pc.CALL_OPTS
    want = ref.calls(alleles, pile, codes, o, region_start=start)
    # conditions on the inputs: 2/3 met with equality (8 of 12) and missed by one read (7 of 11), two alleles at one position, alleles inside
    # an N run that stay silent, an allele on one strand only
    listed = {(a[0], a[1], a[2]): a[3:] for a in ref.listed(alleles)}
    assert [(w[0], w[1], w[3], w[5]) for w in want][:2] == [(250, ref.DEL, 8, 12), (281, ref.INS, 8, 12)] and 8 * o["frac_den"] == o["frac_num"] * 12
    assert listed[(1050, ref.DEL, 4)] == (7, 4) and not any(w[0] == 1050 for w in want) and 7 * o["frac_den"] < o["frac_num"] * 11 <= 8 * o["frac_den"]
    assert sum(pile[1050]["base"][0]) + sum(pile[1050]["base"][1]) + sum(pile[1050]["del"]) == 11
    assert listed[(1550, ref.DEL, 1)] == (4, 2) and listed[(1550, ref.DEL, 3)] == (4, 2)
    assert (65, ref.DEL, 2) in listed and (66, ref.INS, ref.pack([1, 1])) in listed and genome[65] == 4 and genome[66] == 4
    assert listed[(2049, ref.INS, ref.pack([1, 1]))] == (5, 5) and any(w[0] == 2049 for w in want)
    got = _lib.pileup_indel_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"])
    assert _call_tuples(got) == want
    t = _lib.get_timing()
    assert t["fast_path"] == 17 and t["cells"] == len(alleles)
    # the depth is gnx_pileup_calls' depth
    depth = {int(c["pos"]): int(c["depth"]) for c in _lib.pileup_calls(1, 1, 1, 1 << 20, 0)}
    assert all(depth[w[0]] == w[5] for w in want)
    quarter = pc.opts(frac=(1, 4))
    both = ref.calls(alleles, pile, codes, quarter, region_start=start)
    assert [(w[1], w[2]) for w in both if w[0] == 1550] == [(ref.DEL, 1), (ref.DEL, 3)] and any(w[0] == 1050 for w in both)
    for opts in (quarter, pc.opts(min_alt=2, frac=(3, 4)), pc.opts(min_alt=2, frac=(2, 3), both_strands=1), pc.opts(frac=(1, 4), both_strands=1), pc.opts(min_depth=12, min_alt=8),
                 pc.opts(min_depth=13), pc.opts(min_alt=9), pc.opts(frac=(1, 1 << 20)), pc.opts(frac=(1 << 20, 1 << 20))):
        got = _lib.pileup_indel_calls(opts["min_depth"], opts["min_alt"], opts["frac_num"], opts["frac_den"], opts["both_strands"])
        assert _call_tuples(got) == ref.calls(alleles, pile, codes, opts, region_start=start), opts
    assert not any(w[0] == 2049 for w in ref.calls(alleles, pile, codes, pc.opts(frac=(1, 4), both_strands=1), region_start=start))
    assert not any(w[0] in (65, 66) for w in ref.calls(alleles, pile, codes, pc.opts(frac=(1, 1 << 20)), region_start=start))
    public = align.PileupIndelCalls(o["min_depth"], o["min_alt"], frac=(o["frac_num"], o["frac_den"]))
    assert [(d["pos"], d["kind"], d["length"], d["count"], d["count_fwd"], d["depth"], d["ref"]) for d in public] == \
        [(w[0], ("del", "ins", "long_ins")[w[1] - 1], w[2] if w[1] != ref.INS else (w[2].bit_length() + 2) // 3, w[3], w[4], w[5], w[6]) for w in want]
    # the empty result is a pointer all the same
    calls_p, out_n = ctypes.c_void_p(), ctypes.c_int64(-1)
    oc = _lib.GnxPileCallOpts(1000, 1, 1, 2, 0, 0)
    assert _lib.lib().gnx_pileup_indel_calls(ctypes.byref(oc), ctypes.byref(calls_p), ctypes.byref(out_n)) == _lib.GNX_OK and out_n.value == 0 and calls_p.value
    _lib.lib().gnx_free(calls_p)
    _open_tracking(start, n)
    assert _lib.lib().gnx_pileup_indel_calls(ctypes.byref(oc), ctypes.byref(calls_p), ctypes.byref(out_n)) == _lib.GNX_OK and out_n.value == 0 and calls_p.value
    _lib.lib().gnx_free(calls_p)
    assert _lib.lib().gnx_pileup_alleles(ctypes.byref(calls_p), ctypes.byref(out_n)) == _lib.GNX_OK and out_n.value == 0 and calls_p.value
    _lib.lib().gnx_free(calls_p)


# ---- 7. end to end: reports -> tracking pile -> alleles, indel calls, VCF ----
def test_reports_into_alleles_and_vcf(gpu_lib):
    reads = tsg._simulated_reads()
    mx, go, ge = align.DefaultScoreMatrix, -400, -30
    gpu_lib.check(gpu_lib.lib().gnx_set_reference_synthetic(tsg.SYN_LEN, tsg.SYN_SEED))
    try:
        gpu_lib.reference_index_build(tsg.K, 1)
        p = gpu_lib.make_params(sc.LOCAL, mx, go, ge)
        report = align.MapReadsReport(p, reads, tags=True, **tsg.VOTE)
        syn = _lib.synthetic_reference_bases(0, tsg.SYN_LEN, tsg.SYN_SEED)
        region = (0, tsg.SYN_LEN)
        _open_tracking(*region)
        added = align.PileupAddReport(p, reads, report)
        pile, alleles = pyref_pileup.new_pile(tsg.SYN_LEN), ref.new_alleles()
        for rep, read in zip(report, reads):
            if rep["best"] >= 0:
                t_len = sum(r for r, o in rep["route"] if o != sc.I)
                start = rep["window_start"]
                oriented = tsg._rc(read) if rep["strand"] else read
                route = [tuple(c) for c in rep["route"]]
                pyref_pileup.add(pile, sc.LOCAL, start, syn[start:start + t_len], oriented, rep["strand"], route, region)
                ref.add(alleles, start, oriented, rep["strand"], route, region)
        assert added > 50 and (align.PileupGet() == _as_rows(pile)).all()
        want = ref.listed(alleles)
        assert _allele_tuples(_lib.pileup_alleles()) == want
        assert {ref.DEL, ref.INS} <= {w[1] for w in want} and {0, 1} == {rep["strand"] for rep in report if rep["best"] >= 0}
        want_calls = ref.calls(alleles, pile, syn, pc.opts())
        assert _call_tuples(_lib.pileup_indel_calls(1, 1, 1, 2, 0)) == want_calls
        assert {ref.DEL, ref.INS} <= {w[1] for w in want_calls}
        # VCF: the text parses back to the calls
        subs, indels = align.PileupCalls(1, 1), align.PileupIndelCalls(1, 1)
        out = io.StringIO()
        n = vcf.WriteVcf(out, "syn", syn, subs, indels)
        recs = pac.parse_vcf(out.getvalue())
        assert n == len(recs) == sum(1 for c in subs if c["kind"] == "sub") + len(indels)
        letters = "ACGTN"
        back_subs, back_indels = [], []
        for chrom, pos, r, a, info in recs:
            assert chrom == "syn"
            if a == "<INS>":
                back_indels.append((pos - 1, ref.LONG_INS, info["SVLEN"], info["AO"], info["AOF"], info["DP"], letters.index(r)))
            elif len(r) == 1 and len(a) == 1:
                back_subs.append((pos - 1, info["DP"], info["AO"], info["AOF"], letters.index(r), letters.index(a)))
            elif len(a) == 1:
                x = 0 if pos == 1 and a != r[0] else pos  # (a deletion of the first base is anchored behind)
                assert "".join(letters[int(b)] for b in syn[max(x - 1, 0):max(x - 1, 0) + len(r)]) == r and a == (r[0] if x else r[-1])
                back_indels.append((x, ref.DEL, len(r) - 1, info["AO"], info["AOF"], info["DP"], int(syn[x])))
            else:
                assert a[0] == r and len(r) == 1
                back_indels.append((pos - 1, ref.INS, ref.pack(vcf.LettersToBases(a[1:])), info["AO"], info["AOF"], info["DP"], letters.index(r)))
        assert back_subs == [(c["pos"], c["depth"], c["count"], c["count_fwd"], c["ref"], c["alt"]) for c in subs if c["kind"] == "sub"]
        assert sorted(back_indels) == want_calls
        assert [r[1] for r in recs] == sorted(r[1] for r in recs)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 8. the C++ mirror ----
def test_cpp_pile_alleles_mirror_runs(gpu_lib):
    import test_pile_alleles_cpu
    test_pile_alleles_cpu._build_cpp()
    assert subprocess.call([test_pile_alleles_cpu.BIN]) == 0
