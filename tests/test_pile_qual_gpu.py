"""The quality pile and gnx_pileup_genotypes on the device against the literal restatement (tests/pyref_pile_qual.py): counts and quality
sums in both forms of the walk and across sub-batch cuts on the seams of the kernel at every min_baseq that matters, 64 workgroups on
the same counters, the edges of the region, errors that must leave both tables as they were, the life cycle, the genotypes on the
borders of the call kernel (order included), its argument errors, reports end to end into a VCF, and the C++ mirror."""
import ctypes
import functools
import io
import subprocess

import numpy as np
import pytest

import pileup_cases as pc
import pyref_pile_qual as ref
import summary_cases as sc
import test_pileup_gpu as tpg
import test_summary_gpu as tsg
from gonomics_amd import _lib, align, dna, vcf

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
_params, _under = tpg._params, tpg._under


def _quals(reads, salt=0):
    """deterministic qualities: 0, every value around each min_baseq the tests use, 93 and bytes above 93 all occur"""
    return [np.asarray([(7 * j + 3 * (k + salt)) % 101 for j in range(len(r))], dtype=np.uint8) for k, r in enumerate(reads)]


def _restate(region, batch, quals, min_baseq):
    windows, reads, strands, routes = batch
    pile = ref.new_pile(region[1])
    for (start, _), read, q, strand, route in zip(windows, reads, quals, strands, routes):
        ref.add(pile, sc.LOCAL, start, read, q, strand, route, region, min_baseq)
    return pile


def _tables(pile):
    """the restatement's pile as (a PILE_DTYPE array, an int32 [n][4] array)"""
    return tpg._as_rows(pile), np.asarray([r["qsum"] for r in pile], dtype=np.int32).reshape(len(pile), 4)


def _add(p, batch, quals, use=None):
    windows, reads, strands, routes = batch
    align.PileupAdd(p, reads, windows, strands, routes, use=use, quals=quals)


def _both():
    return align.PileupGet(), align.PileupGetQual()


@pytest.fixture
def genome(gpu_lib):
    g, _ = tsg._resident_cases()
    gpu_lib.set_reference(g)
    try:
        yield g
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 1. seams: the summary's hand-made CIGARs as windows of one reference, both strands, every form, cut and min_baseq ----
@functools.lru_cache(maxsize=None)
def _seams(min_baseq):
    g, _ = tsg._resident_cases()
    names, windows, reads, strands, routes = pc.seam_batch(g)
    batch = (windows, reads, strands, routes)
    quals = _quals(reads)
    return batch, quals, _tables(_restate((0, len(g)), batch, quals, min_baseq))


@pytest.mark.parametrize("min_baseq", [0, 1, 20, 93])
def test_seams(gpu_lib, genome, monkeypatch, min_baseq):
    batch, quals, (want, want_q) = _seams(min_baseq)
    seen = set(np.concatenate(quals).tolist())
    assert {0, 1, 2, 19, 20, 21, 92, 93, 94, 100} <= seen  # (conditions on the inputs: the qualities around every threshold, and bytes above 93)
    assert want["base"][:, :, 4].sum() > 0 and want["ins"].sum() > 0 and want["del"].sum() > 0 and want["base"][:, 1].sum() > 0 and want_q.sum() > 0
    p = _params()
    for env in tpg.SWITCHES:
        align.PileupOpen(0, len(genome))
        align.PileupTrackQualities(min_baseq)
        _under(monkeypatch, env, lambda: _add(p, batch, quals))
        got, got_q = _both()
        assert not tpg._differences(got, want, 0), (env, tpg._differences(got, want, 0))
        bad = np.nonzero((got_q != want_q).any(axis=1))[0][:5]
        assert bad.size == 0, (env, [(int(x), got_q[x].tolist(), want_q[x].tolist()) for x in bad])
        t = _lib.get_timing()
        assert t["fast_path"] == 14 and t["cells"] == tpg._columns(batch[3])
        assert align.PileupInfo() == {"start": 0, "len": len(genome), "reads_added": len(batch[0]), "device_bytes": 56 * len(genome)}
        assert align.PileupQualInfo() == {"tracking": True, "min_baseq": min_baseq, "device_bytes": 16 * len(genome)}
    if min_baseq == 0:
        # nothing is cut: the counts are what a plain pile gives for the same batch, and every counted A C G T base has its quality in the sums
        align.PileupOpen(0, len(genome))
        tpg._add(p, batch)
        assert (align.PileupGet() == want).all()
        assert want_q.sum() == sum(min(int(q), 93) for (s, n), rd, qs, route in zip(batch[0], batch[1], quals, batch[3]) for q in _inside_m_quals(rd, qs, route))
    else:
        assert want["base"].sum() < _seams(0)[2][0]["base"].sum()  # (something was cut)
        assert (want["del"] == _seams(0)[2][0]["del"]).all() and (want["ins"] == _seams(0)[2][0]["ins"]).all()  # del and ins do not depend on quality


def _inside_m_quals(read, quals, route):
    """the qualities of the read's A C G T bases in inside M columns (the whole window lies in the region)"""
    import pyref_summary
    cols = pyref_summary.columns(route)
    lead = 0
    while lead < len(cols) and cols[lead] == sc.D:
        lead += 1
    end = len(cols)
    while end > lead and cols[end - 1] == sc.D:
        end -= 1
    j = 0
    for k, c in enumerate(cols):
        if c == sc.M and lead <= k < end and read[j] < 4:
            yield quals[j]
        if c != sc.D:
            j += 1


# ---- 2. contention: 64 workgroups on the same counters ----
def test_contention(gpu_lib, genome, monkeypatch):
    batch = pc.contention_batch(genome)
    quals = [_quals(batch[1][:1])[0]] * len(batch[1])
    want, want_q = _tables(_restate((0, len(genome)), tuple(x[:1] for x in batch), quals[:1], 5))
    assert want["del"].sum() == 1 and want["ins"].sum() == 1 and 100 < want["base"].sum() < 148 and want_q.sum() > 3000
    p = _params()
    for env in tpg.FORMS:
        align.PileupOpen(0, len(genome))
        align.PileupTrackQualities(5)
        _under(monkeypatch, env, lambda: _add(p, batch, quals))
        got, got_q = _both()
        for f in ("base", "del", "ins"):
            assert (got[f] == 256 * want[f]).all(), (env, f)
        assert (got_q == 256 * want_q).all(), env
        assert align.PileupInfo()["reads_added"] == 256


# ---- 3. the edges of the region ----
def test_region_edges(gpu_lib, monkeypatch):
    g = np.zeros(300, np.uint8)
    g[pc.ALPHA_AT:pc.ALPHA_AT + 10] = dna.StringToBases(pc.ALPHA)
    gpu_lib.set_reference(g)
    p = _params()
    try:
        for region in ((0, 300), (104, 3), (109, 40)):
            for strand in (0, 1):
                for (read, route, _), min_baseq in zip(pc.WORKED, (20, 0)):
                    rd = dna.StringToBases(read)
                    quals = [np.asarray([30, 94, 10, 30, 40, 0, 5, 20, 19][:len(rd)], np.uint8)]
                    batch = ([(pc.ALPHA_AT, 10)], [rd], [strand], [route])
                    want, want_q = _tables(_restate(region, batch, quals, min_baseq))
                    for env in tpg.FORMS:
                        align.PileupOpen(*region)
                        align.PileupTrackQualities(min_baseq)
                        _under(monkeypatch, env, lambda: _add(p, batch, quals))
                        got, got_q = _both()
                        assert (got == want).all() and (got_q == want_q).all(), (region, strand, read, env)
        # the batch around the edges of a longer region: counts and sums on both sides of either edge
        genome, _ = tsg._resident_cases()
        gpu_lib.set_reference(genome)
        batch = pc.edge_batch(genome)
        quals = _quals(batch[1], salt=5)
        lo, n = pc.EDGE_REGION
        whole_q = _tables(_restate((0, len(genome)), batch, quals, 20))[1]
        want, want_q = _tables(_restate(pc.EDGE_REGION, batch, quals, 20))
        assert (want_q == whole_q[lo:lo + n]).all() and whole_q[:lo].sum() > 0 and whole_q[lo + n:].sum() > 0 and whole_q[lo:lo + 3].sum() > 0 and whole_q[lo + n - 3:lo + n].sum() > 0
        for env in tpg.FORMS + tpg.CUTS[1:]:
            align.PileupOpen(lo, n)
            align.PileupTrackQualities(20)
            _under(monkeypatch, env, lambda: _add(p, batch, quals))
            got, got_q = _both()
            assert not tpg._differences(got, want, lo) and (got_q == want_q).all(), env
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 4. errors leave both tables as they were ----
@pytest.mark.parametrize("what,code", [("plain_add_on_a_quality_pile", _lib.GNX_EINVAL), ("null_qual_cat", _lib.GNX_EINVAL), ("track_after_an_add", _lib.GNX_EINVAL),
                                       ("byte5_in_a_read", _lib.GNX_EBASE), ("strand_byte_2", _lib.GNX_EINVAL), ("too_much_alpha", _lib.GNX_EINVAL)])
def test_errors_leave_both_tables_as_they_were(gpu_lib, genome, what, code):
    batch, quals, _ = _seams(0)
    p = _params()
    align.PileupOpen(0, len(genome))
    align.PileupTrackQualities(7)
    _add(p, tuple(x[:6] for x in batch), quals[:6])
    before, before_q, info, qinfo = align.PileupGet().tobytes(), align.PileupGetQual().tobytes(), align.PileupInfo(), align.PileupQualInfo()
    assert info["reads_added"] == 6 and np.frombuffer(before_q, np.int32).sum() > 0
    windows, reads, strands, routes = (list(x[:6]) for x in batch)
    q = list(quals[:6])
    last = len(windows)
    # a good pair first and a broken one behind it: nothing of the call may land
    windows.append((500, 20))
    reads.append(np.array(genome[500:520]))
    q.append(np.full(20, 30, np.uint8))
    strands.append(0)
    routes.append([(20, sc.M)])
    if what == "byte5_in_a_read":
        reads[last][7] = 5
    elif what == "strand_byte_2":
        strands[last] = 2
    elif what == "too_much_alpha":
        routes[last] = [(15, sc.M), (6, sc.D), (5, sc.M)]
    with pytest.raises((_lib.GnxError, IndexError)) as ei:
        if what == "plain_add_on_a_quality_pile":
            align.PileupAdd(p, reads, windows, strands, routes)
        elif what == "track_after_an_add":
            align.PileupTrackQualities(0)
        elif what == "null_qual_cat":
            ops, off = align._routes_to_ops(routes)
            cat, roff = _lib._cat(reads)
            _lib.pileup_add_by_offset_qual(p, cat, roff, [w[0] for w in windows], [w[1] for w in windows], strands, ops, off, None)
        else:
            align.PileupAdd(p, reads, windows, strands, routes, quals=q)
    assert (ei.value.__cause__.code if isinstance(ei.value, IndexError) else ei.value.code) == code
    assert align.PileupGet().tobytes() == before and align.PileupGetQual().tobytes() == before_q and align.PileupInfo() == info and align.PileupQualInfo() == qinfo


def test_the_quality_entries_on_a_plain_pile(gpu_lib, genome):
    batch, quals, _ = _seams(0)
    p = _params()
    align.PileupOpen(0, len(genome))
    tpg._add(p, tuple(x[:6] for x in batch))
    before, info = align.PileupGet().tobytes(), align.PileupInfo()
    rows = np.full(8, SENTINEL, np.int64)
    recs, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    for call in (lambda: _add(p, tuple(x[:6] for x in batch), quals[:6]), lambda: align.PileupGetQual(), lambda: align.PileupGenotypes(1), lambda: align.PileupTrackQualities(0)):
        with pytest.raises(_lib.GnxError) as ei:
            call()
        assert ei.value.code == _lib.GNX_EINVAL
    assert _lib.lib().gnx_pileup_get_qual(0, 2, rows.ctypes.data) == _lib.GNX_EINVAL and (rows == SENTINEL).all()
    assert _lib.lib().gnx_pileup_genotypes(ctypes.byref(_lib.GnxGenoOpts(1, 0, 3000, 3300)), ctypes.byref(recs), ctypes.byref(n)) == _lib.GNX_EINVAL
    assert recs.value == SENTINEL and n.value == SENTINEL
    assert align.PileupGet().tobytes() == before and align.PileupInfo() == info and align.PileupQualInfo() == {"tracking": False, "min_baseq": 0, "device_bytes": 0}


# ---- 5. life cycle ----
def test_lifecycle(gpu_lib, genome):
    L = _lib.lib()
    p = _params()
    batch = pc.contention_batch(genome, copies=3)
    quals = _quals(batch[1])
    align.PileupOpen(900, 400)
    assert align.PileupQualInfo() == {"tracking": False, "min_baseq": 0, "device_bytes": 0}
    for q in (-1, 94, 1 << 20):
        assert L.gnx_pileup_track_qualities(q) == _lib.GNX_EINVAL and not align.PileupQualInfo()["tracking"]
    align.PileupTrackQualities(93)
    align.PileupTrackQualities(11)  # (still empty: a second call takes the new threshold)
    assert align.PileupQualInfo() == {"tracking": True, "min_baseq": 11, "device_bytes": 400 * 16}
    assert align.PileupInfo() == {"start": 900, "len": 400, "reads_added": 0, "device_bytes": 400 * 56}
    assert L.gnx_pileup_qual_info(None, None, None) == _lib.GNX_OK
    _add(p, batch, quals)
    want, want_q = _tables(_restate((900, 400), batch, quals, 11))
    got, got_q = _both()
    assert (got == want).all() and (got_q == want_q).all() and got_q.sum() > 0 and align.PileupInfo()["reads_added"] == 3
    # rows outside the region
    rows = np.zeros((401, 4), np.int32)
    for first, count in ((0, 401), (400, 1), (-1, 1), (1, -1), (396, 5)):
        assert L.gnx_pileup_get_qual(first, count, rows.ctypes.data) == _lib.GNX_EINVAL, (first, count)
    assert L.gnx_pileup_get_qual(0, 400, None) == _lib.GNX_EINVAL and L.gnx_pileup_get_qual(400, 0, None) == _lib.GNX_OK
    assert (align.PileupGetQual(100, 7) == want_q[100:107]).all() and align.PileupGetQual(5, 0).shape == (0, 4)
    # open replaces the pile and drops tracking
    align.PileupOpen(1000, 64)
    assert align.PileupQualInfo() == {"tracking": False, "min_baseq": 0, "device_bytes": 0} and align.PileupInfo()["device_bytes"] == 64 * 56
    tpg._add(p, batch)  # (the plain entry is the right one again)
    with pytest.raises(_lib.GnxError):
        align.PileupGetQual()
    # a new reference drops the pile with its planes
    align.PileupOpen(0, 100)
    align.PileupTrackQualities()
    _lib.set_reference(genome[:5000])
    assert L.gnx_pileup_qual_info(None, None, None) == _lib.GNX_EINVAL
    align.PileupOpen(0, 100)
    assert not align.PileupQualInfo()["tracking"]
    align.PileupTrackQualities(3)
    align.PileupClose()
    assert L.gnx_pileup_qual_info(None, None, None) == _lib.GNX_EINVAL
    _lib.set_reference(genome)


def test_allele_and_quality_tracking_together(gpu_lib, genome):
    batch, quals, _ = _seams(20)
    p = _params()
    align.PileupOpen(0, len(genome))
    align.PileupTrackAlleles()
    tpg._add(p, batch)
    plain = align.PileupAlleles()
    plain_norm = align.PileupAlleles(normalize=True)
    assert len(plain) > 3 and {a["kind"] for a in plain} >= {"del", "ins"}
    want, want_q = _seams(20)[2]
    for order in (0, 1):
        align.PileupOpen(0, len(genome))
        for step in ((align.PileupTrackAlleles, lambda: align.PileupTrackQualities(20)) if order == 0 else (lambda: align.PileupTrackQualities(20), align.PileupTrackAlleles)):
            step()
        assert align.PileupAlleleInfo()["tracking"] and align.PileupQualInfo()["tracking"]
        _add(p, batch, quals)
        for got, exp in ((align.PileupAlleles(), plain), (align.PileupAlleles(normalize=True), plain_norm)):
            assert len(got) == len(exp)
            for a, b in zip(got, exp):
                assert {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in a.items()} == {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        got, got_q = _both()
        assert (got == want).all() and (got_q == want_q).all()


# ---- 6. genotypes on the kernel's borders ----
CLASSES = ("hom_ref", "het", "hom_alt", "triallelic", "low_quality_alt", "shallow", "one_bad_alt")
EMITS = {"het": 1, "hom_alt": 2, "triallelic": 1, "low_quality_alt": 1}  # the genotype at min_depth 3 and the default priors, by the header's arithmetic


def _site_reads(x, c, cls):
    """the single-base reads over position x (reference code c; over an N the `reference` reads say A): (base, quality, strand) each"""
    r = c if c < 4 else 0
    a1, a2 = (r + 1 + x % 3) % 4, (r + 1 + (x + 1) % 3) % 4
    if cls == "hom_ref":
        plan = [(r, 30, 12)]
    elif cls == "het":
        plan = [(r, 30, 6), (a1, 31, 6)]
    elif cls == "hom_alt":
        plan = [(a1, 30, 12)]
    elif cls == "triallelic":
        plan = [(r, 30, 5), (a1, 30, 5), (a2, 35, 4)]
    elif cls == "low_quality_alt":  # L = (13 540, 12 030, 48 070): two thirds alt by count, and no alt / alt call -- ref / alt at qual 1 510
        plan = [(a1, 2, 20), (r, 40, 10)]
    elif cls == "one_bad_alt":      # L[0] = 677: ref / ref
        plan = [(r, 30, 11), (a1, 2, 1)]
    else:
        plan = [(a1, 30, 2)]
    return [(b, q, k % 2) for b, q, n in plan for k in range(n)]


def _site_batch(genome, start, n, cls_of):
    windows, reads, strands, routes, quals = [], [], [], [], []
    for x in range(start, start + n):
        for b, q, s in _site_reads(x, int(genome[x]), cls_of(x - start)):
            windows.append((x, 1))
            reads.append(np.array([b], np.uint8))
            quals.append(np.array([q], np.uint8))
            strands.append(s)
            routes.append([(1, sc.M)])
    return (windows, reads, strands, routes), quals


def _geno_tuples(recs):
    return [(int(g["pos"]), int(g["gt"]), int(g["ref"]), int(g["alt"]), [int(v) for v in g["pl"]], int(g["gq"]), int(g["qual"]), int(g["depth"]), int(g["ref_count"]),
             int(g["alt_count"]), int(g["alt_fwd"])) for g in recs]


def _want_tuples(recs):
    return [(g["pos"], g["gt"], g["ref"], g["alt"], g["pl"], g["gq"], g["qual"], g["depth"], g["ref_count"], g["alt_count"], g["alt_fwd"]) for g in recs]


GENO_OPTS = [ref.opts(3), ref.opts(3, 1500), ref.opts(1, 0, 0, 0), ref.opts(13, 0, 0, 1 << 20), ref.opts(3, 0, 1 << 20, 0)]


def _check_genotypes(genome, start, n, pile, expect_some=True):
    for o in GENO_OPTS:
        want = ref.genotypes(pile, genome[start:start + n], o, region_start=start)
        got = _lib.pileup_genotypes(o["min_depth"], o["min_qual"], o["prior_het"], o["prior_hom"])
        assert _geno_tuples(got) == _want_tuples(want), (start, n, o)
        assert (got["_pad"] == 0).all()
        t = _lib.get_timing()
        assert t["fast_path"] == 20 and t["cells"] == n
    return ref.genotypes(pile, genome[start:start + n], GENO_OPTS[0], region_start=start)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_genotypes_on_the_borders(gpu_lib, genome, n):
    p = _params()
    # 48: on a 16-base word boundary of the packed reference, the N run 60 .. 70 from the region's 13th position; 37: off it; 4000: the second N run at 90 .. 100
    for start in (48, 37, 4000):
        special = {0, n - 1, 63, 64, 255, 256} | {k for k in range(n) if 58 <= start + k <= 71 or 4088 <= start + k <= 4101}  # variants there: het and hom alternating
        cls_of = lambda k: ("het", "hom_alt")[k % 2] if k in special else CLASSES[(k * 5 + 1) % 7]
        batch, quals = _site_batch(genome, start, n, cls_of)
        pile = _restate((start, n), batch, quals, 0)
        align.PileupOpen(start, n)
        align.PileupTrackQualities(0)
        _add(p, batch, quals)
        got, got_q = _both()
        want, want_q = _tables(pile)
        assert (got == want).all() and (got_q == want_q).all()
        recs = _check_genotypes(genome, start, n, pile)
        at = {g["pos"]: g for g in recs}
        # conditions on the inputs: the variants on the borders are called, a variant under an N is silent and the one beside it is not
        for k in sorted(special):
            x = start + k
            if 0 <= k < n:
                assert (x in at) == (genome[x] < 4), (start, n, x)
                if x in at:
                    assert at[x]["gt"] == (1, 2)[k % 2], (start, n, x)
        if n >= 63:
            classes = {cls_of(k) for k in range(n)}
            assert classes == set(CLASSES)
            for k in range(n):
                x, cls = start + k, cls_of(k)
                if genome[x] < 4 and k not in special:
                    assert (at[x]["gt"] if x in at else 0) == EMITS.get(cls, 0), (x, cls)
                    if cls == "low_quality_alt":
                        assert at[x]["qual"] == 1510 and at[x]["alt_count"] == 20 and at[x]["ref_count"] == 10
        if n >= 63 and start == 48:
            assert genome[60] == 4 and 60 not in at and 59 in at and 70 in at


def test_genotypes_none_and_all(gpu_lib, genome):
    p = _params()
    start, n = 100, 200
    assert (genome[start:start + n] < 4).all()
    # no record at all: every position hom-ref, one bad alt base or shallow
    batch, quals = _site_batch(genome, start, n, lambda k: ("hom_ref", "one_bad_alt", "shallow")[k % 3])
    pile = _restate((start, n), batch, quals, 0)
    align.PileupOpen(start, n)
    align.PileupTrackQualities(0)
    _add(p, batch, quals)
    assert _check_genotypes(genome, start, n, pile) == []
    recs, cnt = ctypes.c_void_p(), ctypes.c_int64(-1)
    assert _lib.lib().gnx_pileup_genotypes(ctypes.byref(_lib.GnxGenoOpts(3, 0, 3000, 3300)), ctypes.byref(recs), ctypes.byref(cnt)) == _lib.GNX_OK and cnt.value == 0 and recs.value
    _lib.lib().gnx_free(recs)
    assert align.PileupGenotypes(3) == []
    # every position emits: all 64 lanes of every step write
    batch, quals = _site_batch(genome, start, n, lambda k: ("het", "hom_alt", "triallelic")[k % 3])
    pile = _restate((start, n), batch, quals, 0)
    align.PileupOpen(start, n)
    align.PileupTrackQualities(0)
    _add(p, batch, quals)
    got = _check_genotypes(genome, start, n, pile)
    assert [g["pos"] for g in got] == list(range(start, start + n))
    assert align.PileupGenotypes(3) == [dict(g) for g in got]
    # min_baseq cuts the q2 bases before they are counted: the same reads, another pile
    batch, quals = _site_batch(genome, start, n, lambda k: "low_quality_alt")
    pile = _restate((start, n), batch, quals, 3)
    align.PileupOpen(start, n)
    align.PileupTrackQualities(3)
    _add(p, batch, quals)
    assert align.PileupGet()["base"].sum() == 10 * n and _check_genotypes(genome, start, n, pile) == []


# ---- 7. argument errors of gnx_pileup_genotypes ----
@pytest.mark.parametrize("bad", [(0, 0, 3000, 3300), (1, -1, 3000, 3300), (1, 0, -1, 3300), (1, 0, (1 << 20) + 1, 3300), (1, 0, 3000, -1), (1, 0, 3000, (1 << 20) + 1), "null_opts", "null_out", "null_n"], ids=str)
def test_genotype_argument_errors(gpu_lib, genome, bad):
    align.PileupOpen(0, 100)
    align.PileupTrackQualities(0)
    recs, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    o = _lib.GnxGenoOpts(*bad) if isinstance(bad, tuple) else _lib.GnxGenoOpts(1, 0, 3000, 3300)
    rc = _lib.lib().gnx_pileup_genotypes(None if bad == "null_opts" else ctypes.byref(o), None if bad == "null_out" else ctypes.byref(recs), None if bad == "null_n" else ctypes.byref(n))
    assert rc == _lib.GNX_EINVAL and recs.value == SENTINEL and n.value == SENTINEL
    assert align.PileupGenotypes(1, 0, 0, 1 << 20) == []  # (the ends of the ranges are inside)


# ---- 8. end to end: reads with qualities -> reports -> the quality pile -> genotypes -> VCF ----
E2E_LEN, E2E_K = 4096, 16
E2E_HOM, E2E_HET = (400, 1111, 2048, 3003), (640, 1500, 1501, 2600, 3500)


def _sample():
    """a reference, the sample's two haplotypes (planted SNPs: hom on both, het on the second), and a tiling of 100-base reads, one every 4
    bases, alternating haplotype and strand, error-free but for one q2 miscall in every third read; qualities 25 .. 40 elsewhere"""
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, size=E2E_LEN).astype(np.uint8)
    haps = [genome.copy(), genome.copy()]
    for x in E2E_HOM:
        haps[0][x] = haps[1][x] = (genome[x] + 1) % 4
    for x in E2E_HET:
        haps[1][x] = (genome[x] + 2) % 4
    reads, quals = [], []
    for k, s in enumerate(range(0, E2E_LEN - 100 + 1, 4)):
        rd = haps[k % 2][s:s + 100].copy()
        q = np.asarray([25 + (3 * j + k) % 16 for j in range(100)], np.uint8)
        if k % 3 == 0:
            at = (k * 7) % 100
            rd[at] = (rd[at] + 1 + k % 3) % 4
            q[at] = 2
        if (k // 2) % 2:
            rd, q = tsg._rc(rd), q[::-1].copy()
        reads.append(rd)
        quals.append(q if k % 5 else "".join(chr(33 + int(v)) for v in q))  # (every fifth as an ASCII + 33 string)
    return genome, reads, quals


def test_reads_with_qualities_into_genotypes_and_vcf(gpu_lib):
    genome, reads, quals = _sample()
    gpu_lib.set_reference(genome)
    try:
        gpu_lib.reference_index_build(E2E_K, 1)
        p = gpu_lib.make_params(sc.LOCAL, align.DefaultScoreMatrix, -400, -30)
        report = align.MapReadsReport(p, reads, tags=True, **tsg.VOTE)
        region, min_mapq, min_baseq = (0, E2E_LEN), 20, 10
        align.PileupOpen(*region)
        align.PileupTrackQualities(min_baseq)
        added = align.PileupAddReport(p, reads, report, min_mapq=min_mapq, quals=quals)
        pile = ref.new_pile(E2E_LEN)
        n = 0
        for rep, read, q in zip(report, reads, quals):
            if rep["best"] >= 0 and rep["mapq"] >= min_mapq:
                q = align._phred(q)
                ref.add(pile, sc.LOCAL, rep["window_start"], tsg._rc(read) if rep["strand"] else read, q[::-1] if rep["strand"] else q, rep["strand"], [tuple(c) for c in rep["route"]], region, min_baseq)
                n += 1
        assert added == n == align.PileupInfo()["reads_added"] and n > 0.9 * len(reads) and {rep["strand"] for rep in report if rep["best"] >= 0} == {0, 1}
        want, want_q = _tables(pile)
        got, got_q = _both()
        assert (got == want).all() and (got_q == want_q).all()
        genos = align.PileupGenotypes(8, min_qual=2000)
        exp = ref.genotypes(pile, genome, ref.opts(8, 2000))
        assert genos == [{k: g[k] for k in genos[0]} for g in exp]
        # the planted sites come back with the planted genotype, and nothing else does
        assert {g["pos"]: (g["gt"], g["alt"]) for g in genos} == dict([(x, (2, (genome[x] + 1) % 4)) for x in E2E_HOM] + [(x, (1, (genome[x] + 2) % 4)) for x in E2E_HET])
        out, out_exp = io.StringIO(), io.StringIO()
        assert vcf.WriteGenotypeVcf(out, "syn", genome, genos) == len(E2E_HOM) + len(E2E_HET) == vcf.WriteGenotypeVcf(out_exp, "syn", genome, exp)
        assert out.getvalue() == out_exp.getvalue()
        lines = [ln.split("\t") for ln in out.getvalue().split("\n") if ln and not ln.startswith("#")]
        assert [int(f[1]) - 1 for f in lines] == sorted(E2E_HOM + E2E_HET) and all(f[8] == "GT:GQ:PL:AD" and f[9].split(":")[0] == ("1/1" if int(f[1]) - 1 in E2E_HOM else "0/1") for f in lines)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


# ---- 9. the C++ mirror ----
def test_cpp_pile_qual_mirror_runs(gpu_lib):
    import test_pile_qual_cpu
    test_pile_qual_cpu._build_cpp()
    assert subprocess.call([test_pile_qual_cpu.BIN]) == 0
