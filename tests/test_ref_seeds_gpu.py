"""The k-mer index of the resident reference and candidate windows by seed votes (gnx_reference_index_*, gnx_seed_candidates,
align.SeedCandidates / align.MapReads) against the plain-Python restatement tests/pyref_seeds.py.  Every comparison is exact equality:
index keys and positions, all five candidate arrays, every field of the composed call."""
import ctypes
import functools

import numpy as np
import pytest

import pyref_seeds
from gonomics_amd import _lib, align

pytestmark = pytest.mark.gpu
K = 16
BASE = dict(max_occ=16, bin=32, pad=16, max_cand=4, min_votes=2)
N_RUN = (4096 - 35, 4096 + 35)  # straddles a flag-word edge and a 64-base block edge of the packed form
BAD_BYTE, DUP_SRC, DUP_DST, DUP_LEN, HOMO, HOMO_LEN = 12000, 6000, 15000, 300, 17000, 400


@functools.lru_cache(maxsize=None)
def fixture_ref():
    rng = np.random.default_rng(20260)
    ref = rng.integers(0, 4, 20000).astype(np.uint8)
    ref[N_RUN[0]:N_RUN[1]] = 4
    ref[BAD_BYTE] = 7
    ref[DUP_DST:DUP_DST + DUP_LEN] = ref[DUP_SRC:DUP_SRC + DUP_LEN]
    ref[HOMO:HOMO + HOMO_LEN] = 0
    ref.setflags(write=False)
    return ref


def _rc(x):
    x = np.asarray(x, np.uint8)[::-1].copy()
    m = x < 4
    x[m] = 3 - x[m]
    return x


def _substitute(rng, x, n):
    x = x.copy()
    for p in rng.choice(x.shape[0], size=n, replace=False):
        x[p] = (x[p] + rng.integers(1, 4)) % 4 if x[p] < 4 else x[p]
    return x


def _sample(rng, ref, n, lo=0, hi=None):
    hi = ref.shape[0] - n if hi is None else hi
    while True:
        s = int(rng.integers(lo, hi + 1))
        if not np.any(ref[s:s + n] >= 5):  # (a read may hold an N, never a byte >= 5)
            return s


@functools.lru_cache(maxsize=None)
def sub_reads():
    """400 reads of 150 bases from both strands with 0-3 substitutions"""
    rng, ref, out = np.random.default_rng(7), fixture_ref(), []
    for i in range(400):
        s = _sample(rng, ref, 150)
        x = _substitute(rng, ref[s:s + 150], int(rng.integers(0, 4)))
        out.append(_rc(x) if i & 1 else x)
    return out


@functools.lru_cache(maxsize=None)
def indel_reads():
    """the same with one indel of 1-5 bases"""
    rng, ref, out = np.random.default_rng(8), fixture_ref(), []
    for i in range(400):
        s = _sample(rng, ref, 156)
        x = _substitute(rng, ref[s:s + 156], int(rng.integers(0, 4)))
        at, ln = int(rng.integers(20, 130)), int(rng.integers(1, 6))
        x = np.concatenate([x[:at], x[at + ln:]]) if rng.integers(0, 2) else np.concatenate([x[:at], rng.integers(0, 4, ln).astype(np.uint8), x[at:150 - ln]])
        out.append(_rc(x) if i & 1 else x)
    return out


@functools.lru_cache(maxsize=None)
def special_reads():
    rng, ref = np.random.default_rng(9), fixture_ref()
    with_n = ref[2000:2150].copy()
    with_n[75] = 4
    half = ref[3000:3075]
    return [ref[100:100 + K - 1], ref[100:100 + K], ref[100:101],                       # lengths k - 1, k, 1
            with_n,                                                                      # an N in the middle
            np.concatenate([rng.integers(0, 4, 40).astype(np.uint8), ref[:110]]),        # its first 40 bases precede position 0: negative diagonals
            np.concatenate([ref[-100:], rng.integers(0, 4, 50).astype(np.uint8)]),       # overhangs the reference end
            ref[DUP_SRC + 50:DUP_SRC + 200].copy(),                                      # the duplicated segment: equal votes, the order falls to the bin
            _rc(ref[DUP_SRC + 50:DUP_SRC + 200]),                                        # ... on the other strand
            np.concatenate([half, _rc(half)]),                                           # equal to its own reverse complement: the order falls to the strand
            np.zeros(150, np.uint8),                                                     # homopolymer: more entries than BASE's max_occ
            ref[N_RUN[0] - 60:N_RUN[0] + 90].copy()]                                     # runs into the N run


def suite_reads():
    return sub_reads() + indel_reads() + special_reads()


_STATE = [None]


@pytest.fixture(scope="module", autouse=True)
def _fresh_state():
    _STATE[0] = None
    yield
    _STATE[0] = None


def _resident(lib, name, ref, k, step):
    """make `ref` resident with its index of (k, step), unless the module left exactly that behind"""
    if _STATE[0] != (name, k, step):
        _STATE[0] = None
        lib.set_reference(ref)
        lib.reference_index_build(k, step)
        _STATE[0] = (name, k, step)


@functools.lru_cache(maxsize=None)
def _fixture_table(k, step):
    return pyref_seeds.lookup_table(pyref_seeds.index(fixture_ref(), k, step))


def _expected(table, ref_len, k, reads, opts):
    per_read = [pyref_seeds.candidates(ref_len, table, k, r, **opts) for r in reads]
    flat = [c for cs in per_read for c in cs]
    off = np.concatenate([[0], np.cumsum([len(cs) for cs in per_read])]).astype(np.int64)
    return (off, np.asarray([c[0] for c in flat], np.int64), np.asarray([c[1] for c in flat], np.int64), np.asarray([c[2] for c in flat], np.uint8),
            np.asarray([c[3] for c in flat], np.int32)), per_read


def _same(got, exp, what):
    for name, g, e in zip(("cand_off", "cand_start", "cand_len", "cand_strand", "cand_votes"), got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:5] if g.shape == e.shape else (g.shape, e.shape))


def _run(lib, reads, opts):
    cat, off = lib._cat([np.asarray(r, np.uint8) for r in reads])
    return lib.seed_candidates(cat, off, **opts)


@pytest.fixture(params=["default", "slab"])
def placement(request, monkeypatch):
    """where the vote tables live: the library's own choice, or every read in a slab of device memory"""
    monkeypatch.delenv("GNX_SEED_SUB", raising=False)
    if request.param == "slab":
        monkeypatch.setenv("GNX_SEED_VOTE_LDS", "0")
    else:
        monkeypatch.delenv("GNX_SEED_VOTE_LDS", raising=False)
    return request.param


# ---- the index ----
def _check_index(lib, ref, k, step, what):
    lib.set_reference(ref)
    _STATE[0] = None
    lib.reference_index_build(k, step)
    keys, pos = lib.reference_index_get()
    exp = pyref_seeds.index(ref, k, step)
    assert keys.dtype == np.uint64 and pos.dtype == np.uint64
    assert keys.tolist() == [c for c, _ in exp], what
    assert pos.tolist() == [p for _, p in exp], what
    info = lib.reference_index_info()
    assert info["device_bytes"] >= 16 * len(exp)
    assert (info["n_kmers"], info["seed_len"], info["seed_step"]) == (len(exp), k, step), what


@pytest.mark.parametrize("step", [1, 3, 16])
@pytest.mark.parametrize("k", [8, 16, 31, 32])
def test_index_equals_restatement(gpu_lib, k, step):
    """k = 32 fills all 64 key bits; the prefix of 4 097 bases ends just behind a flag-word edge inside the N run"""
    ref = fixture_ref()
    for length in (k - 1, k, k + 1, 63, 64, 65, 4097, ref.shape[0]):
        _check_index(gpu_lib, ref[:length], k, step, (k, step, length))


def test_a_reference_of_no_bases_is_none(gpu_lib):
    gpu_lib.set_reference(fixture_ref())
    gpu_lib.reference_index_build(K, 1)
    gpu_lib.set_reference(np.zeros(0, np.uint8))  # releases the reference, and the index with it
    _STATE[0] = None
    L = gpu_lib.lib()
    assert L.gnx_reference_index_build(K, 1) == gpu_lib.GNX_EINVAL
    assert L.gnx_reference_index_info(None, None, None, None) == gpu_lib.GNX_EINVAL
    with pytest.raises(gpu_lib.GnxError) as ei:
        _run(gpu_lib, special_reads()[:2], BASE)
    assert ei.value.code == gpu_lib.GNX_EINVAL


@pytest.mark.parametrize("k", [16, 32])
def test_index_skips_what_is_no_base_at_every_edge(gpu_lib, k):
    """an N or a byte >= 5 at the first base, the last base and either side of a 16-base word edge and of a 64-base block edge"""
    base = np.random.default_rng(k).integers(0, 4, 200).astype(np.uint8)
    for at in (0, 199, 15, 16, 63, 64, 127, 128):
        for val in (4, 9):
            ref = base.copy()
            ref[at] = val
            _check_index(gpu_lib, ref, k, 1, (k, at, val))
    ref = base.copy()
    ref[60:70] = 4
    ref[63] = 200
    ref[130] = 5
    _check_index(gpu_lib, ref, k, 3, (k, "runs"))


@pytest.mark.parametrize("step", [1, 3])
def test_index_built_in_many_compaction_passes(gpu_lib, monkeypatch, step):
    monkeypatch.setenv("GNX_REF_INDEX_SUB", "1000")
    _check_index(gpu_lib, fixture_ref(), K, step, ("passes of 1000 positions", step))


# ---- candidates ----
OPTION_SETS = {"base": {}, "max_cand_1": {"max_cand": 1}, "max_cand_2": {"max_cand": 2}, "max_cand_64": {"max_cand": 64, "min_votes": 1}, "min_votes_1": {"min_votes": 1},
               "min_votes_20": {"min_votes": 20}}


@functools.lru_cache(maxsize=None)
def _suite_expected(name, step):
    opts = dict(BASE, **OPTION_SETS[name])
    return _expected(_fixture_table(K, step), fixture_ref().shape[0], K, suite_reads(), opts)[0], opts


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_candidates_equal_restatement(gpu_lib, placement, name):
    exp, opts = _suite_expected(name, 1)
    _resident(gpu_lib, "fixture", fixture_ref(), K, 1)
    _same(_run(gpu_lib, suite_reads(), opts), exp, (placement, name))
    t = gpu_lib.get_timing()
    assert t["fast_path"] == 11 and t["cells"] > 0 and t["n_launches"] >= 1


def test_candidates_with_an_index_of_every_third_position(gpu_lib, placement):
    exp, opts = _suite_expected("min_votes_1", 3)
    _resident(gpu_lib, "fixture", fixture_ref(), K, 3)
    _same(_run(gpu_lib, suite_reads(), opts), exp, placement)


def test_homopolymer_at_the_occurrence_limit(gpu_lib, placement):
    """max_occ set to exactly the number of entries of the homopolymer's k-mer, and to one less"""
    table = _fixture_table(K, 1)
    occ = len(table[0])
    assert occ >= HOMO_LEN - K + 1
    reads = [np.zeros(150, np.uint8), np.full(150, 3, np.uint8), sub_reads()[0]]
    _resident(gpu_lib, "fixture", fixture_ref(), K, 1)
    for max_occ, some in ((occ, True), (occ - 1, False)):
        opts = dict(BASE, max_occ=max_occ, max_cand=64, min_votes=1)
        exp, per_read = _expected(table, fixture_ref().shape[0], K, reads, opts)
        assert bool(per_read[0]) == some and bool(per_read[1]) == some
        _same(_run(gpu_lib, reads, opts), exp, (placement, max_occ))


def test_empty_batch_and_reads_without_candidates(gpu_lib, placement):
    _resident(gpu_lib, "fixture", fixture_ref(), K, 1)
    off, start, ln, strand, votes = _run(gpu_lib, [], BASE)
    assert off.tolist() == [0] and start.shape == (0,) and votes.shape == (0,)
    rng = np.random.default_rng(1)
    reads = [np.zeros(0, np.uint8), rng.integers(0, 4, 150).astype(np.uint8), np.full(40, 4, np.uint8), np.zeros(3, np.uint8)]
    off, start, ln, strand, votes = _run(gpu_lib, reads, BASE)
    assert off.tolist() == [0, 0, 0, 0, 0] and start.shape == (0,)


def test_a_batch_that_uses_both_table_forms(gpu_lib, monkeypatch):
    """ordinary reads vote in LDS; a 2 000-base read over the duplicated segment has more hits than the LDS table takes"""
    monkeypatch.delenv("GNX_SEED_VOTE_LDS", raising=False)
    monkeypatch.delenv("GNX_SEED_SUB", raising=False)
    ref = fixture_ref()
    reads = sub_reads()[:20] + [ref[DUP_SRC - 1000:DUP_SRC + 1000].copy()] + sub_reads()[20:30]
    opts = dict(BASE, max_cand=8, min_votes=1)
    _resident(gpu_lib, "fixture", ref, K, 1)
    gpu_lib.debug_counter(7, reset=True)
    gpu_lib.debug_counter(8, reset=True)
    got = _run(gpu_lib, reads, opts)
    in_lds, in_slab = gpu_lib.debug_counter(7, reset=True), gpu_lib.debug_counter(8, reset=True)
    assert in_lds > 0 and in_slab > 0 and in_lds + in_slab <= len(reads), (in_lds, in_slab)
    _same(got, _expected(_fixture_table(K, 1), ref.shape[0], K, reads, opts)[0], "mixed")


def test_sub_batch_cuts_change_nothing(gpu_lib, placement, monkeypatch):
    reads = sub_reads()
    _resident(gpu_lib, "fixture", fixture_ref(), K, 1)
    whole = _run(gpu_lib, reads, BASE)
    t = gpu_lib.get_timing()
    assert t["n_launches"] == 1 and t["cells"] > 0, t
    monkeypatch.setenv("GNX_SEED_SUB", str(t["cells"] // 6))
    cut = _run(gpu_lib, reads, BASE)
    t2 = gpu_lib.get_timing()
    assert t2["n_launches"] >= 5 and t2["cells"] == t["cells"], t2
    _same(cut, whole, "cut into at least five")
    monkeypatch.setenv("GNX_SEED_SUB", "1")  # a cut between any two reads
    few = _run(gpu_lib, reads[:40], BASE)
    assert gpu_lib.get_timing()["n_launches"] >= 30
    _same(few, _expected(_fixture_table(K, 1), fixture_ref().shape[0], K, reads[:40], BASE)[0], "one read per launch")


# ---- lifetime ----
def _refused(lib, reads):
    with pytest.raises(lib.GnxError) as ei:
        _run(lib, reads, BASE)
    return ei.value.code


def test_index_lives_and_dies_with_the_reference(gpu_lib):
    ref, reads = fixture_ref(), sub_reads()[:30]
    _STATE[0] = None
    gpu_lib.set_reference(ref)
    assert _refused(gpu_lib, reads) == gpu_lib.GNX_EINVAL  # candidates before any build
    gpu_lib.reference_index_build(K, 1)
    exp = _expected(_fixture_table(K, 1), ref.shape[0], K, reads, BASE)[0]
    _same(_run(gpu_lib, reads, BASE), exp, "first build")
    other = np.roll(ref, 5000).copy()
    other[other > 4] = 4
    gpu_lib.set_reference(other)  # another sequence of the same length: the old index must not answer for it
    assert _refused(gpu_lib, reads) == gpu_lib.GNX_EINVAL
    assert gpu_lib.lib().gnx_reference_index_info(None, None, None, None) == gpu_lib.GNX_EINVAL
    gpu_lib.reference_index_build(K, 1)
    table = pyref_seeds.lookup_table(pyref_seeds.index(other, K, 1))
    exp_other = _expected(table, other.shape[0], K, reads, BASE)[0]
    assert not np.array_equal(exp_other[1], exp[1])
    _same(_run(gpu_lib, reads, BASE), exp_other, "rebuilt on the new sequence")
    gpu_lib.reference_index_build(12, 2)  # a second build replaces the first
    assert gpu_lib.reference_index_info()["seed_len"] == 12
    table = pyref_seeds.lookup_table(pyref_seeds.index(other, 12, 2))
    _same(_run(gpu_lib, reads, BASE), _expected(table, other.shape[0], 12, reads, BASE)[0], "second build")
    gpu_lib.check(gpu_lib.lib().gnx_set_reference_synthetic(5000, 3))  # the synthetic reference drops it as well
    assert _refused(gpu_lib, reads) == gpu_lib.GNX_EINVAL
    gpu_lib.reference_index_build(K, 1)
    keys, pos = gpu_lib.reference_index_get()
    exp_idx = pyref_seeds.index(gpu_lib.synthetic_reference_bases(0, 5000, 3), K, 1)
    assert keys.tolist() == [c for c, _ in exp_idx] and pos.tolist() == [p for _, p in exp_idx]


def test_the_graph_aligner_keeps_its_seed_index_and_generation(gpu_lib):
    L = gpu_lib.lib()
    nodes = [fixture_ref()[100:400].copy(), fixture_ref()[500:700].copy()]
    keys, locs = gpu_lib.seed_index_build(nodes, 12, 1)
    ncat, noff = gpu_lib._cat(nodes)
    gen = ctypes.c_uint64()
    gpu_lib.check(L.gnx_seed_index_set_gen(keys.ctypes.data, locs.ctypes.data, keys.shape[0], ncat.ctypes.data, noff.ctypes.data, len(nodes), 12, ctypes.byref(gen)))
    rcat, roff = gpu_lib._cat([fixture_ref()[150:250].copy(), fixture_ref()[520:600].copy()])

    def find():
        hp, op = ctypes.c_void_p(), ctypes.c_void_p()
        gpu_lib.check(L.gnx_seed_find_batch_gen(gen.value, rcat.ctypes.data, roff.ctypes.data, 2, ctypes.byref(hp), ctypes.byref(op)))
        off = np.ctypeslib.as_array(ctypes.cast(op, ctypes.POINTER(ctypes.c_int64)), shape=(3,)).copy()
        raw = ctypes.string_at(hp.value, int(off[-1]) * gpu_lib.SEED_HIT_DTYPE.itemsize) if off[-1] else b""
        L.gnx_free(hp)
        L.gnx_free(op)
        return off.tolist(), raw
    before = find()
    assert before[0][-1] > 0
    _STATE[0] = None
    gpu_lib.set_reference(fixture_ref())
    gpu_lib.reference_index_build(K, 1)
    _run(gpu_lib, sub_reads()[:10], BASE)
    gpu_lib.reference_index_build(K, 3)
    assert find() == before  # same generation, same hits


# ---- reads in, placements out ----
@functools.lru_cache(maxsize=None)
def plain_reads():
    """200 substitution-only reads from the plain part of the fixture, with strand and origin"""
    rng, ref, out = np.random.default_rng(11), fixture_ref(), []
    for i in range(200):
        s = int(rng.integers(7000, 11000))
        x = _substitute(rng, ref[s:s + 150], int(rng.integers(0, 4)))
        out.append((_rc(x) if i & 1 else x, i & 1, s))
    return out


@pytest.mark.parametrize("mode", [_lib.GNX_AFFINE_GAP_LOCAL, _lib.GNX_AFFINE_GAP], ids=["local", "global"])
def test_map_reads_equals_best_of_on_the_restatements_candidates(gpu_lib, mode):
    ref = fixture_ref()
    reads = [r for r, _, _ in plain_reads()]
    _resident(gpu_lib, "fixture", ref, K, 1)
    params = gpu_lib.make_params(mode, align.DefaultScoreMatrix, -400, -30)
    per_read = _expected(_fixture_table(K, 1), ref.shape[0], K, reads, dict(BASE))[1]
    got = align.MapReads(params, reads, **BASE)
    exp = align.MapBestOf(params, reads, [[(s, l, st) for s, l, st, _ in cs] for cs in per_read])
    assert len(got) == len(exp) == 200
    for r, (g, e) in enumerate(zip(got, exp)):
        assert g[:5] == e, r
        best = g[0]
        assert best >= 0, r
        w_start, w_len, w_strand, _ = per_read[r][best]
        assert g[5] == w_start, r
        _, strand, origin = plain_reads()[r]
        # all surviving seeds of such a read lie on the diagonal of its origin, and the window of that bin covers the read's interval
        assert w_strand == strand and w_start <= origin and origin + 150 <= w_start + w_len, (r, per_read[r], strand, origin)
    assert align.SeedCandidates(reads[:5], **BASE) == per_read[:5]
