"""The graph aligner's seed index and seed search (csrc/seed_kernels.hip.h, the gnx_seed_* entries, and their host statements in
gonomics_amd/genomeGraph.py and include/gonomics_genomegraph.hpp) on the adversarial case of tests/gsw_adversarial.py, against the
restatement tests/pyref_gsw.py.  All comparisons are exact equality.  The reference's own tests of this path only log: PARITY UNPINNED.

What the case holds, by the restatement (gsw_adversarial.census; 23 nodes, 34 reads), per (seed_len, step):

    setting   raw hits  seeds    reads > 100 seeds  locations of the fullest key  right > 64  left stops at read start  border entries
    (2, 5)     100 804  100 804  32                  56                            2 915       15 115                      2
    (8, 1)     128 985  128 985  19                 212                           13 438       61 386                     50
    (16, 1)     96 655   96 655  14                 188                           11 910       45 753                    106
    (31, 3)     17 501   17 501   9                  49                            3 016        8 176                     61
    (32, 1)     48 156   48 156   9                 140                            8 854       22 969                    187
    (32, 32)     2 431    2 431   5                   7                              347          779                      4

Whole reads (test_reads_on_the_adversarial_graph), decided by the restatement: at (16, 1) 20 reads have <= 100 seeds and 16 of them map
with AlnScore > 0; at (32, 1) 25 and 18.  The Go code panics on none of them."""
import ctypes
import functools

import numpy as np
import pytest

import common
import gsw_adversarial as adv
import pyref_gsw as ref
from gonomics_amd import genomeGraph as gg

MX = common.matrices()
READS_SETTINGS = ((16, 1), (32, 1))
READS_FLOOR = {(16, 1): (20, 16), (32, 1): (25, 18)}  # (reads with <= 100 seeds, of which mapped), measured with the restatement on the CPU


def build(seqs, edges):
    g = gg.GenomeGraph()
    for k, s in enumerate(seqs):
        gg.AddNode(g, gg.Node(k, s))
    for u, v in edges:
        gg.AddEdge(g.Nodes[u], g.Nodes[v])
    return g


@functools.lru_cache(maxsize=None)
def graph():
    seqs, edges, _, _ = adv.case()
    return build(seqs, edges)


def bigs():
    return [gg.FastqBig("r%d" % k, rd) for k, rd in enumerate(adv.case()[2])]


def host_raw_hits(index, gnodes, big, seed_len):
    """pyref_gsw.raw_hits assembled from the product's host functions"""
    out = []
    rb, rbrc = big.rainbows()
    for rs in range(0, len(big.Seq) - seed_len + 1):
        for st, rain in ((0, rb), (1, rbrc)):
            for code in index.get(gg._read_key(rain, rs, seed_len), []):
                nid, npos = gg.numberToChromAndPos(code)
                ro = 31 - ((rs - npos % 32 + 31) % 32)
                lm = min(rs + 1, gg.CountLeftMatches(gnodes[nid].SeqTwoBit, npos, rain[ro], rs + ro))
                q, ns = rs - (lm - 1), npos - (lm - 1)
                ro = 31 - ((q - ns % 32 + 31) % 32)
                out.append((rs, st, nid, ns, q, gg.CountRightMatches(gnodes[nid].SeqTwoBit, ns, rain[ro], q + ro)))
    return out


# ---- CPU: the product's host statement against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("setting", adv.SETTINGS, ids=lambda s: "k%d_step%d" % s)
def test_host_raw_hits_on_the_adversarial_case(setting):
    """index, two-bit words with the N quirk, CountLeftMatches / CountRightMatches and the clamp, hit for hit"""
    seed_len, step = setting
    g = graph()
    idx = gg.IndexGenomeIntoMap(g.Nodes, seed_len, step)
    assert idx == adv.ref_index(seed_len, step)
    exp = adv.ref_raw_hits(seed_len, step)
    for k, big in enumerate(bigs()):
        assert host_raw_hits(idx, g.Nodes, big, seed_len) == exp[k], "read %d" % k


@pytest.mark.parametrize("setting", adv.SETTINGS, ids=lambda s: "k%d_step%d" % s)
def test_host_seed_map_on_the_adversarial_case(setting):
    """gg.seed_map_host == ref.seed_map on the whole case: the continuation across node borders in both directions and the seed order"""
    seed_len, step = setting
    g = graph()
    idx = adv.ref_index(seed_len, step)
    exp = adv.ref_seeds(seed_len, step)
    for k, big in enumerate(bigs()):
        assert [s.key() for s in gg.seed_map_host(idx, g.Nodes, big, seed_len)] == exp[k], "read %d" % k


# ---- GPU: index and raw hits ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("setting", adv.SETTINGS, ids=lambda s: "k%d_step%d" % s)
def test_device_index_and_raw_hits(gpu_lib, setting):
    seed_len, step = setting
    g = graph()
    reads = adv.case()[2]
    full = adv.ref_index(seed_len, step)
    exp = adv.ref_raw_hits(seed_len, step)
    index = gg.SeedIndex(g.Nodes, seed_len, step)
    ks = sorted(full)
    assert [int(x) for x in index.keys] == [k for k in ks for _ in full[k]]
    assert [int(x) for x in index.locs] == [v for k in ks for v in full[k]]  # the map's insertion order within a key, border k-mers merged in
    node_seqs = [n.Seq for n in g.Nodes]
    got = gpu_lib.seed_find_batch(index.keys, index.locs, node_seqs, reads, seed_len)
    assert len(got) == len(reads)
    for k in range(len(reads)):
        assert got[k] == exp[k], "read %d" % k
    # batch-independent: the same reads in reversed order (zero-slot reads first instead of last, another longest-read word count per
    # position in the batch) ...
    rev = gpu_lib.seed_find_batch(index.keys, index.locs, node_seqs, reads[::-1], seed_len)
    assert rev[::-1] == exp
    # ... and each read alone in a batch of one (RW = the read's own word count)
    for k, rd in enumerate(reads):
        assert gpu_lib.seed_find_batch(index.keys, index.locs, node_seqs, [rd], seed_len) == [exp[k]], "read %d alone" % k


# ---- GPU: seeds and whole reads ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("setting", READS_SETTINGS, ids=lambda s: "k%d_step%d" % s)
def test_seeds_on_the_adversarial_graph(gpu_lib, setting):
    """gg.seed_map_batch (device hits, continuation across node borders on the host, the documented stable order above 100 seeds) ==
    ref.seed_map for EVERY read"""
    seed_len, step = setting
    g = graph()
    exp = adv.ref_seeds(seed_len, step)
    index = gg.SeedIndex(g.Nodes, seed_len, step)
    got = gg.seed_map_batch(index, g.Nodes, bigs(), seed_len)
    assert len(got) == len(exp)
    for k in range(len(exp)):
        assert [s.key() for s in got[k]] == exp[k], "read %d" % k


@pytest.mark.gpu
@pytest.mark.parametrize("setting", READS_SETTINGS, ids=lambda s: "k%d_step%d" % s)
def test_reads_on_the_adversarial_graph(gpu_lib, setting):
    """GswBatchToGiraf of the Python mirror == ref.read_to_giraf, and the native read path (1 and 5 host threads) == the Python mirror,
    for the reads with at most 100 seeds.  The cut is decided by the restatement alone and is there for time: a read with 25 000 seeds
    takes minutes in the sequential restatement."""
    seed_len, step = setting
    g = graph()
    nodes = adv.ref_graph()
    sc = MX["HumanChimpTwo"]
    seeds = adv.ref_seeds(seed_len, step)
    keep = [k for k in range(len(seeds)) if len(seeds[k]) <= 100]
    all_bigs = bigs()
    some = [all_bigs[k] for k in keep]
    index = gg.SeedIndex(g.Nodes, seed_len, step)
    got = gg.GswBatchToGiraf(g, some, index, seed_len, sc, on_panic="mark")
    mapped = 0
    for x, k in enumerate(keep):
        try:
            exp = ref.read_to_giraf(nodes, adv.ref_reads()[k], seeds[k], sc)
        except IndexError:  # the Go code panics on this read (search.go:139)
            assert isinstance(got[x], gg.GoPanic), "read %d" % k
            continue
        assert got[x].key() == ref.giraf_key(exp), "read %d" % k
        mapped += exp["AlnScore"] > 0
    print("setting %r: %d reads with <= 100 seeds, %d mapped" % (setting, len(keep), mapped))
    assert (len(keep), mapped) == READS_FLOOR[setting] and len(keep) >= 15 and mapped >= 10
    ng = gg.NativeGraph(g, seed_len, step)
    try:
        for threads in (1, 5):
            nat = ng.GswBatchToGiraf(some, sc, threads=threads, on_panic="mark")
            assert len(nat) == len(got)
            for x, (a, b) in enumerate(zip(nat, got)):
                if isinstance(b, gg.GoPanic):
                    assert isinstance(a, gg.GoPanic), "read %d" % keep[x]
                else:
                    assert a.key() == b.key() and a.Flag == b.Flag and a.MapQ == b.MapQ, "read %d (%d threads)" % (keep[x], threads)
    finally:
        ng.handle.close()


# ---- GPU: who owns the device's ONE resident index -----------------------------------------------------------------------------------
def _other_graph(seed):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (90, 45, 130)]
    reads = [np.concatenate([seqs[0][60:], seqs[1][:30]]), seqs[2][10:80].copy(), seqs[2][40:120].copy()]
    return seqs, [(0, 1), (1, 2)], reads


def _same_map(a, b):
    """two results of GswGraph.map_reads, field by field (the bytes behind a cigar's op are padding)"""
    return (a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist()
            and a[2]["run_length"].tolist() == b[2]["run_length"].tolist() and a[2]["op"].tolist() == b[2]["op"].tolist())


@pytest.mark.gpu
def test_resident_index_after_other_indexes(gpu_lib):
    """search index 1, let something else take or invalidate the device's resident index, search index 1 again with the SAME arguments
    (one node_seqs list object): the ctypes mirror's "my index is resident" must not outlive the device's.  And the other way round
    for a graph handle: a bare index build in between must cost it an upload, not an error."""
    seed_len, step = 32, 32
    g = graph()
    reads = adv.case()[2]
    exp = adv.ref_raw_hits(seed_len, step)
    index = gg.SeedIndex(g.Nodes, seed_len, step)
    node_seqs = [n.Seq for n in g.Nodes]
    sc = MX["HumanChimpTwo"]

    def find():
        return gpu_lib.seed_find_batch(index.keys, index.locs, node_seqs, reads, seed_len)

    assert find() == exp
    assert find() == exp  # (resident: no upload)
    o_seqs, o_edges, o_reads = _other_graph(3)
    keys, _ = gpu_lib.seed_index_build(o_seqs, 16, 1)  # invalidates the resident index (it uploads its nodes into the same buffers)
    assert keys.shape[0] > 0
    assert find() == exp
    h = gpu_lib.GswGraph(o_seqs, o_edges, 16, 1)  # builds an index inside
    h.close()
    assert find() == exp
    h = gpu_lib.GswGraph(o_seqs, o_edges, 16, 1)
    try:
        first = h.map_reads(o_reads, sc)  # the handle's index becomes the resident one
        o_nodes = ref.make_graph(o_seqs, o_edges)
        o_full = ref.index_genome(o_nodes, 16, 1)
        o_exp = [ref.read_to_giraf(o_nodes, r2, ref.seed_map(o_full, o_nodes, r2, 16), sc) for r2 in (ref.make_read(rd) for rd in o_reads)]
        assert [int(x) for x in first[0]["aln_score"]] == [e["AlnScore"] for e in o_exp] and all(e["AlnScore"] > 0 for e in o_exp)
        assert find() == exp
        again = h.map_reads(o_reads, sc)  # ... and the handle's after the raw entries took the device back
        assert _same_map(first, again)
        with pytest.raises(gpu_lib.GnxError):
            h.map_reads(o_reads + [np.full(20, 7, np.uint8)], sc)  # a base >= 5: refused
        assert find() == exp
        gpu_lib.seed_index_build(o_seqs, 16, 1)  # a bare build between two batches of the handle
        again = h.map_reads(o_reads, sc)
        assert _same_map(first, again)
        assert find() == exp
    finally:
        h.close()


@pytest.mark.gpu
def test_alternating_graphs_of_equal_shape(gpu_lib):
    """two graphs with identical node lengths and different bases, alternated through gg.seed_map_batch (which hands a temporary node
    list to the library every time: ids of temporaries repeat)"""
    shapes = (70, 33, 64, 120)
    edges = [(0, 1), (1, 2)]
    cases = []
    for seed in (21, 22):
        rng = np.random.default_rng(seed)
        seqs = [rng.integers(0, 4, size=n).astype(np.uint8) for n in shapes]
        reads = [np.concatenate([seqs[0][30:], seqs[1], seqs[2][:20]]), seqs[3][5:100].copy(), seqs[2].copy()]
        g, nodes = build(seqs, edges), ref.make_graph(seqs, edges)
        full = ref.index_genome(nodes, 16, 1)
        exp = [ref.seed_map(full, nodes, ref.make_read(rd), 16) for rd in reads]
        assert all(len(e) > 0 for e in exp)
        cases.append((g, gg.SeedIndex(g.Nodes, 16, 1), [gg.FastqBig("r", rd) for rd in reads], exp))
    assert cases[0][1].keys.shape == cases[1][1].keys.shape  # (no N, same lengths: same number of k-mers)
    for turn in range(6):
        g, index, rds, exp = cases[turn % 2]
        got = gg.seed_map_batch(index, g.Nodes, rds, 16)
        assert [[s.key() for s in per] for per in got] == exp, "turn %d" % turn


# ---- GPU: edges of the three entries -------------------------------------------------------------------------------------------------
def _raw_find(L, reads):
    """gnx_seed_find_batch as the C ABI has it, against whatever is resident -> (rc, hit offsets or None)"""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    if reads:
        off[1:] = np.cumsum([len(r) for r in reads])
    cat = np.ascontiguousarray(np.concatenate([np.asarray(r, np.uint8) for r in reads] + [np.zeros(1, np.uint8)]))
    hp, op = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.gnx_seed_find_batch(cat.ctypes.data, off.ctypes.data, len(reads), ctypes.byref(hp), ctypes.byref(op))
    hoff = None
    if rc == 0:
        hoff = np.ctypeslib.as_array(ctypes.cast(op, ctypes.POINTER(ctypes.c_int64)), shape=(len(reads) + 1,)).copy()
        if hp.value:
            L.gnx_free(hp)
        L.gnx_free(op)
    return rc, hoff


@pytest.mark.gpu
def test_seed_entry_edges(gpu_lib):
    L = gpu_lib.lib()
    rng = np.random.default_rng(9)
    R = lambda n: rng.integers(0, 4, size=n).astype(np.uint8)  # noqa: E731
    reads = [R(40), R(16), np.zeros(0, np.uint8), R(3)]
    # no node reaches seed_len: an empty index; set with n_index = 0, then a search
    short = [R(10), R(15), R(1)]
    keys, locs = gpu_lib.seed_index_build(short, 16, 1)
    assert keys.shape == (0,) and locs.shape == (0,)
    assert gpu_lib.seed_find_batch(keys, locs, short, reads, 16) == [[], [], [], []]
    rc, hoff = _raw_find(L, reads)
    assert rc == 0 and hoff.tolist() == [0, 0, 0, 0, 0]
    # ... the same nodes in a chain: every index entry is a k-mer across node borders (the device builds none of them, it searches all)
    sedges = [(0, 1), (1, 2)]
    g, nodes = build(short, sedges), ref.make_graph(short, sedges)
    full = ref.index_genome(nodes, 16, 1)
    index = gg.SeedIndex(g.Nodes, 16, 1)
    assert index.keys.shape[0] == sum(len(v) for v in full.values()) > 0
    crd = [np.concatenate(short), np.concatenate(short)[3:24]]
    got = gpu_lib.seed_find_batch(index.keys, index.locs, short, crd, 16)
    assert got == [ref.raw_hits(full, nodes, ref.make_read(rd), 16) for rd in crd] and all(len(x) > 0 for x in got)
    # all reads shorter than the seed, and no reads at all, against a real index
    seqs = [R(80), R(50)]
    keys, locs = gpu_lib.seed_index_build(seqs, 16, 1)
    assert keys.shape[0] == 65 + 35
    assert gpu_lib.seed_find_batch(keys, locs, seqs, [R(15), np.zeros(0, np.uint8), R(1)], 16) == [[], [], []]
    assert gpu_lib.seed_find_batch(keys, locs, seqs, [], 16) == []
    rc, hoff = _raw_find(L, [])
    assert rc == 0 and hoff.tolist() == [0]
    assert len(gpu_lib.seed_find_batch(keys, locs, seqs, [seqs[0][10:60]], 16)[0]) >= 35  # (the index is there and finds)
    # a read beyond the entry's limit of 100 000 bases
    with pytest.raises(gpu_lib.GnxError) as e:
        gpu_lib.seed_find_batch(keys, locs, seqs, [R(20), np.zeros(100001, np.uint8)], 16)
    assert e.value.code == gpu_lib.GNX_EINVAL
    assert len(gpu_lib.seed_find_batch(keys, locs, seqs, [np.zeros(100000, np.uint8), seqs[1]], 16)[1]) >= 35
    # a search with no index set: the build took the resident index' buffers
    keys2, _ = gpu_lib.seed_index_build(seqs, 20, 3)
    assert keys2.shape[0] > 0
    rc, hoff = _raw_find(L, [seqs[0][:40]])
    assert rc == gpu_lib.GNX_EINVAL and hoff is None
    assert b"no resident seed index" in L.gnx_last_error()
    assert len(gpu_lib.seed_find_batch(keys, locs, seqs, [seqs[0][10:60]], 16)[0]) >= 35  # (and the library goes on)
