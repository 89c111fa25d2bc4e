"""Every reader of the packed resident reference on every window class of tests/packed_ref.py.

The reference is kept as 2 bits per base, one flag bit per 64-base block that holds anything but A C G T, a rank per 4 096-base flag
word and two masks per flagged block, and six separate pieces of block / word / rank arithmetic read it in place: BetaSrcT::init / value
(the headline sweep, the score, local and span sweeps, the summary, MD and pile kernels), fp_cert_kernel<true>, ref_kmer_clean /
ref_kmer_key, norm_chunk and its kin, the window unpackers, and the writers that every one of them depends on.  An off-by-one in any of
them changes results only for windows on a block, flag-word or end border -- in a genome the borders of N runs and the contig ends.

Every expected value comes from the BYTES: ref[s:s + l] handed to the CPU oracle or to the entry's pyref_* specification, never from
another GPU call; where an entry has a byte-window twin the twin must agree as well.  Every comparison is equality.  Route switches and
route numbers are those of tests/test_scratch_state_gpu.py (ROUTES / ROUTE_SWITCHES, imported).  test_every_class_ran: no class and no
entry of the table was skipped when the module runs whole."""
import functools

import numpy as np
import pytest

import common
import oracle
import packed_ref as pr
import pyref_seeds
from test_scratch_state_gpu import ROUTES, ROUTE_SWITCHES, _apply, _route_is

pytestmark = pytest.mark.gpu

MX = common.matrices()[pr.MX_NAME]
GO, GE = pr.GO, pr.GE
READBACK = [[10, 20, 30, 40, 50]] + [list(r) for r in MX[1:]]  # row A: five distinct values, all above any route with a gap
RAN = set()


@pytest.fixture(autouse=True)
def _own_switches(monkeypatch):
    for k in ROUTE_SWITCHES + ("GNX_REF_UNPACK", "GNX_RCCL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")


@pytest.fixture
def main(gpu_lib):
    g = pr.main_ref()
    gpu_lib.set_reference(g)
    try:
        assert gpu_lib.reference_info()[0] == len(g) and gpu_lib.reference_info()[2] == pr.flagged_blocks(g)
        yield g
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def _cat(seqs):
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return np.concatenate([np.asarray(x, np.uint8) for x in seqs] + [np.zeros(1, np.uint8)]), off


def _tables(wins):
    return np.asarray([w[0] for w in wins], np.int64), np.asarray([w[1] for w in wins], np.int64)


def _slices(ref, wins):
    return [ref[s:s + l] for s, l in wins]


def _routes_of(res):
    _, ops, off = res
    return [[(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])] for k in range(len(off) - 1)]


# ---- the read-back: every base through the unpacker, the headline sweep and the score sweep ---------------------------------------------------
def _read_back(L, monkeypatch, pos, want_bytes, what, two_contexts=False):
    """one-base reads "A" against one-base windows: pair x scores READBACK[A][ref[x]]"""
    pos = np.asarray(pos, np.int64)
    n = pos.shape[0]
    want = np.asarray(READBACK[0], np.int64)[np.minimum(want_bytes, 4)]
    a_cat, a_off, one = np.zeros(n + 1, np.uint8), np.arange(n + 1, dtype=np.int64), np.ones(n, np.int64)
    p = L.make_params(L.GNX_AFFINE_GAP, READBACK, GO, GE)
    for env, route in ((ROUTES["stored_hform/small/mode0"].env, 0), (ROUTES["fast_path/1_blocks/global"].env, 1)):
        with monkeypatch.context() as mp:
            _apply(mp, env)
            sc, ops, off = L.align_batch_by_offset(p, a_cat, a_off, pos, one)
            tm = L.get_timing()
        _route_is(tm, route, what)
        assert not two_contexts or tm["n_contexts"] == 2
        assert np.array_equal(sc, want), (what, "align", route, pos[np.flatnonzero(sc != want)[:8]])
        assert np.array_equal(off, np.arange(n + 1)) and (ops["run_length"] == 1).all() and (ops["op"] == 0).all(), (what, route)
    sc = L.score_batch_by_offset(p, a_cat, a_off, pos, one)
    tm = L.get_timing()
    assert tm["fast_path"] == 7 and (not two_contexts or tm["n_contexts"] == 2), (what, tm)
    assert np.array_equal(sc, want), (what, "score", pos[np.flatnonzero(sc != want)[:8]])


def test_read_back_every_base_of_main(gpu_lib, monkeypatch, main):
    wins = pr.windows("every_base")
    pos = np.asarray([s for s, _ in wins], np.int64)
    _read_back(gpu_lib, monkeypatch, pos, main[pos], "main")
    RAN.add(("every_base", "read_back"))


@pytest.mark.parametrize("ln", pr.ENDS_LENGTHS)
def test_read_back_ends(gpu_lib, monkeypatch, ln):
    try:
        for variant in pr.ENDS_VARIANTS:
            g = pr.ends_refs()[(ln, variant)]
            gpu_lib.set_reference(g)
            assert gpu_lib.reference_info()[0] == ln and gpu_lib.reference_info()[2] == pr.flagged_blocks(g), (ln, variant)
            _read_back(gpu_lib, monkeypatch, np.arange(ln), g, ("ends", ln, variant))
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    RAN.add(("ends_%d" % ln, "read_back"))


def test_read_back_synthetic_across_the_pack_pass(gpu_lib, monkeypatch):
    """300 000 500 bases in two passes of 2^28: the ranks carried over the border, an exception run behind it, the end inside that run"""
    L = gpu_lib
    try:
        L.check(L.lib().gnx_set_reference_synthetic(pr.SYN_LEN, pr.SYN_SEED))
        runs = [(50000000 * k, min(50000000 * k + 1000, pr.SYN_LEN)) for k in range(1, 7)]
        assert L.reference_info()[0] == pr.SYN_LEN and L.reference_info()[2] == sum((hi - 1) // 64 - lo // 64 + 1 for lo, hi in runs)
        pos = pr.syn_positions()
        _read_back(L, monkeypatch, pos, L.synthetic_reference_positions(pos, pr.SYN_SEED), "synthetic")
    finally:
        L.check(L.lib().gnx_set_reference_synthetic(0, pr.SYN_SEED))
    RAN.add(("synthetic", "read_back"))


# ---- align ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _align_expected(name, blocks, mode):
    return oracle.align_batch(mode, MX, GO, GE, pr.reads(name, blocks), _slices(pr.main_ref(), pr.windows(name)), threads=8)


def _admitted_in(g, wins, reads, packed=True):
    """(reads without N, reads with N) that the certificate admits on the packed reference: the host statement of what the kernel
    decides (the rule that takes reads with N), and fp_cert_kernel<true>'s own condition -- no flagged block under the window
    (BetaSrcT::init's `dirty`, restated in the catalogue); packed=False: on byte windows, the host statement alone"""
    from gonomics_amd import _lib
    p = _lib.make_params(_lib.GNX_AFFINE_GAP, MX, GO, GE)
    layout = pr.pack(g)
    plain = with_n = 0
    for r, (s, l) in zip(reads, wins):
        out = _lib.debug_gapless_certificate_n(p, r, g[s:s + l])
        if out[0] and not (packed and pr.dirty(layout, s, l)):
            plain, with_n = plain + (out[5] == 0), with_n + (out[5] > 0)
    return plain, with_n


@functools.lru_cache(maxsize=None)
def _admitted(name, packed=True):
    return _admitted_in(pr.main_ref(), pr.windows(name), pr.reads(name), packed)


FAST, GENERAL = ROUTES["fast_path/1_blocks/global"].env, ROUTES["stored_hform/small/mode0"].env
ALIGN_ROUTES = {  # name: (switches, reads of how many row blocks, mode, route)
    "default": ({}, 1, 0, None),  # windows of fewer than 768 columns, or a mixed small batch: the unpacker and the stored matrix
    "fast_path/certificate_off": (dict(FAST, GNX_FP_CERT="0"), 1, 0, 1),
    "fast_path/certificate_on": (dict(FAST), 1, 0, 1),
    "fast_path/certificate_forced": (ROUTES["fast_path/certificate_forced"].env, 1, 0, 1),
    "fast_path/row_blocks": (dict(FAST), 2, 0, 1),
    "general": (GENERAL, 1, 0, 0),
    "latency": (dict(ROUTES["latency/small/mode0"].env, GNX_REF_UNPACK="1"), 1, 0, 3),  # (a packed beta never takes this geometry: unpacked first)
    "snapshot16": (dict(ROUTES["snapshot16/static/mode0/checker10000"].env, GNX_FASTPATH="0"), 1, 0, 2),
    "snapshot64": (dict(ROUTES["snapshot64/farm/mode0/checker10000"].env, GNX_FASTPATH="0"), 1, 0, 6),
    "unpacked": ({"GNX_REF_UNPACK": "1"}, 1, 0, None),
    "local_window_as_beta": ({}, 1, 3, 0),
}
assert ROUTES["latency/small/mode0"].align[-1] == 3 and ROUTES["snapshot16/static/mode0/checker10000"].align[-1] == 2
assert ROUTES["snapshot64/farm/mode0/checker10000"].align[-1] == 6 and ROUTES["fast_path/1_blocks/global"].align[-1] == 1


def _default_route_of(wins, reads):
    """the router's rule for a batch of fewer than 8 192 pairs with GNX_FP_SMALL=1: the fast path takes windows of 768 columns and more,
    all reads of one number of row blocks -- else the stored matrix"""
    return 1 if all(l >= 768 for _, l in wins) and len({(len(r) + 159) // 160 for r in reads}) == 1 else 0


def _default_route(name):
    return _default_route_of(pr.windows(name), pr.reads(name))


@pytest.mark.parametrize("how", list(ALIGN_ROUTES))
@pytest.mark.parametrize("name", pr.RUN_CLASSES)
def test_align(gpu_lib, monkeypatch, main, name, how):
    L = gpu_lib
    env, blocks, mode, route = ALIGN_ROUTES[how]
    _apply(monkeypatch, env)
    reads = pr.reads(name, blocks)
    cat, off = _cat(reads)
    ws, wl = _tables(pr.windows(name))
    for c in (9, 10, 11):
        L.debug_counter(c)
    got = L.align_batch_by_offset(L.make_params(mode, MX, GO, GE), cat, off, ws, wl)
    tm = L.get_timing()
    common.assert_same(got, _align_expected(name, blocks, mode), "%s, %s" % (name, how))
    _route_is(tm, _default_route(name) if route is None else route, (name, how))
    assert tm["n_contexts"] == 1
    if how == "fast_path/certificate_forced":
        assert (L.debug_counter(9), L.debug_counter(11), L.debug_counter(10)) == _admitted(name) + (len(reads),), name
        if name == "clean_edges":  # counter 9 is positive where the catalogue says so: one more or one fewer dirty window would show
            assert 4 * _admitted(name)[0] >= len(reads) and pr.certificate_counts()[0] > 0  # the device certifies its quarter here
    elif how in ("fast_path/certificate_off", "general"):
        assert L.debug_counter(10) == 0  # nothing was offered to the certificate
    for c in (9, 10, 11):
        L.debug_counter(c)
    twin = L.align_batch_windows(L.make_params(mode, MX, GO, GE), cat, off[:-1], np.diff(off), main, ws, wl)
    common.assert_same(got, twin, "%s, %s: the byte-window twin" % (name, how))
    if how == "fast_path/certificate_forced":  # on bytes there is no `dirty`: the host statement alone
        assert (L.debug_counter(9), L.debug_counter(11), L.debug_counter(10)) == _admitted(name, packed=False) + (len(reads),), name
    RAN.add((name, "align/" + how))


# ---- the windows of `ends`: the whole reference, its last min(L, 70) bases, its last base ------------------------------------------------------
ENDS_ALIGN = ("default", "fast_path/certificate_forced", "general", "unpacked", "local_window_as_beta")


@functools.lru_cache(maxsize=None)
def _ends_expected(ln, variant):
    import pyref_span
    wins = _slices(pr.ends_refs()[(ln, variant)], pr.ends_windows(ln))
    reads = pr.ends_reads(ln, variant)
    return {0: oracle.align_batch(0, MX, GO, GE, reads, wins, threads=8), 3: oracle.align_batch(3, MX, GO, GE, reads, wins, threads=8),
            "spans": pyref_span.spans_from_oracle(MX, GO, GE, wins, reads, threads=8)}


def _tiled(res, rep):
    """an oracle result for the batch repeated `rep` times"""
    sc, ops, off = res
    return np.tile(sc, rep), np.tile(ops, rep), np.concatenate([off[:1]] + [off[1:] + r * off[-1] for r in range(rep)])


def _ends_every_entry(L, monkeypatch, ln, variant, rep=1, contexts=1):
    """align on five routes (counters exact under the forced certificate), score, locate and span on the three windows of one `ends`
    reference, which is resident; each with its byte-window twin"""
    g, wins, reads, exp = pr.ends_refs()[(ln, variant)], pr.ends_windows(ln), pr.ends_reads(ln, variant), _ends_expected(ln, variant)
    what = ("ends", ln, variant, contexts)
    cat, off = _cat(list(reads) * rep)
    ws, wl = _tables(list(wins) * rep)
    for how in ENDS_ALIGN:
        env, _, mode, route = ALIGN_ROUTES[how]
        p = L.make_params(mode, MX, GO, GE)
        with monkeypatch.context() as mp:
            _apply(mp, env)
            for c in (9, 10, 11):
                L.debug_counter(c)
            got = L.align_batch_by_offset(p, cat, off, ws, wl)
            tm = L.get_timing()
            counters = (L.debug_counter(9), L.debug_counter(11), L.debug_counter(10))
            twin = L.align_batch_windows(p, cat, off[:-1], np.diff(off), g, ws, wl)
        common.assert_same(got, _tiled(exp[mode], rep), "%s, %s" % (what, how))
        common.assert_same(twin, got, "%s, %s: the byte-window twin" % (what, how))
        _route_is(tm, _default_route_of(wins, reads) if route is None else route, (what, how))
        assert tm["n_contexts"] == contexts, (what, how)
        if how == "fast_path/certificate_forced" and contexts == 1:
            assert counters == _admitted_in(g, wins, reads) + (len(ws),), what
    for mode in (0, 3):
        p = L.make_params(mode, MX, GO, GE)
        want = np.tile(np.asarray(exp[mode][0], np.int64), rep)
        got = L.score_batch_by_offset(p, cat, off, ws, wl)
        tm = L.get_timing()
        assert tm["fast_path"] == (7 if mode == 0 else 8) and tm["n_contexts"] == contexts, (what, mode, tm["fast_path"], tm["n_contexts"])
        assert np.array_equal(got, want), (what, "score", mode, np.flatnonzero(got != want)[:8])
        assert np.array_equal(L.score_batch_windows(p, cat, off[:-1], np.diff(off), g, ws, wl), want), (what, "score twin", mode)
    S, start, end = (np.tile(x, rep) for x in exp["spans"])
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, MX, GO, GE)
    for fn in (lambda: L.locate_batch_by_offset(p, cat, off, ws, wl), lambda: L.locate_batch_windows(p, g, ws, wl, cat, off[:-1], np.diff(off))):
        sc, en = fn()
        assert L.get_timing()["fast_path"] == 8, what
        assert np.array_equal(sc, S) and np.array_equal(en, end), (what, "locate")
    for fn in (lambda: L.locate_span_batch_by_offset(p, cat, off, ws, wl), lambda: L.locate_span_batch_windows(p, g, ws, wl, cat, off[:-1], np.diff(off))):
        sc, st, en = fn()
        assert L.get_timing()["fast_path"] == 10, what
        assert np.array_equal(sc, S) and np.array_equal(st, start) and np.array_equal(en, end), (what, "span")


@pytest.mark.parametrize("ln", pr.ENDS_LENGTHS)
def test_ends_windows(gpu_lib, monkeypatch, ln):
    """real windows with their reads that end on the last base of a reference of 1 .. 8 192 bases: the last dword of the certificate's
    grid and of the unpackers, BetaSrcT's look-ahead and its look-up one block past the end in the padding words"""
    try:
        for variant in pr.ENDS_VARIANTS:
            gpu_lib.set_reference(pr.ends_refs()[(ln, variant)])
            _ends_every_entry(gpu_lib, monkeypatch, ln, variant)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    RAN.add(("ends_%d" % ln, "windows"))


# ---- score, locate, span ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spans(name):
    import pyref_span
    return pyref_span.spans_from_oracle(MX, GO, GE, _slices(pr.main_ref(), pr.windows(name)), pr.reads(name), threads=8)


@pytest.mark.parametrize("name", pr.RUN_CLASSES)
def test_score_locate_span(gpu_lib, main, name):
    L = gpu_lib
    reads = pr.reads(name)
    cat, off = _cat(reads)
    ws, wl = _tables(pr.windows(name))
    for mode in (0, 3):  # (the local mode's beta is the window here, as in the align entry)
        p = L.make_params(mode, MX, GO, GE)
        exp = np.asarray(_align_expected(name, 1, mode)[0], np.int64)
        got = L.score_batch_by_offset(p, cat, off, ws, wl)
        assert L.get_timing()["fast_path"] == (7 if mode == 0 else 8), (name, mode, L.get_timing()["fast_path"])
        assert np.array_equal(got, exp), (name, "score", mode, np.flatnonzero(got != exp)[:8])
        twin = L.score_batch_windows(p, cat, off[:-1], np.diff(off), main, ws, wl)
        assert np.array_equal(twin, exp), (name, "score twin", mode)
    RAN.add((name, "score"))
    S, start, end = _spans(name)
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, MX, GO, GE)
    for what, fn in (("by_offset", lambda: L.locate_batch_by_offset(p, cat, off, ws, wl)),
                     ("windows", lambda: L.locate_batch_windows(p, main, ws, wl, cat, off[:-1], np.diff(off)))):
        sc, en = fn()
        assert L.get_timing()["fast_path"] == 8, (name, what)
        assert np.array_equal(sc, S) and np.array_equal(en, end), (name, "locate", what, np.flatnonzero((sc != S) | (en != end))[:8])
    RAN.add((name, "locate"))
    for what, fn in (("by_offset", lambda: L.locate_span_batch_by_offset(p, cat, off, ws, wl)),
                     ("windows", lambda: L.locate_span_batch_windows(p, main, ws, wl, cat, off[:-1], np.diff(off)))):
        sc, st, en = fn()
        assert L.get_timing()["fast_path"] == 10, (name, what)
        assert np.array_equal(sc, S) and np.array_equal(st, start) and np.array_equal(en, end), (name, "span", what, np.flatnonzero((sc != S) | (st != start) | (en != end))[:8])
    RAN.add((name, "span"))


# ---- best of K and best pair, on both strands ------------------------------------------------------------------------------------------------
CAND_CLASSES = ("beside_n", "to_the_end", "start_mod")


@functools.lru_cache(maxsize=None)
def _best_of_case(name):
    """every read of the class with its own window on both strands and its neighbour's window"""
    import test_best_of_gpu as bo
    wins, reads = pr.windows(name), pr.reads(name)
    reads = [bo._rc(r) if k % 2 else r for k, r in enumerate(reads)]
    cands = []
    for k, w in enumerate(wins):
        right, wrong, beside = w + (k % 2,), w + (1 - k % 2,), wins[(k + 1) % len(wins)] + (k % 2,)
        cands.append([right, wrong, beside] if k % 4 < 2 else [wrong, beside, right])
    return reads, cands


@functools.lru_cache(maxsize=None)
def _best_of_expected(name, mode):
    import test_best_of_gpu as bo
    reads, cands = _best_of_case(name)
    return bo._expected(mode, MX, GO, GE, reads, pr.main_ref(), cands)


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("name", CAND_CLASSES)
def test_best_of(gpu_lib, main, name, mode):
    import test_best_of_gpu as bo
    L = gpu_lib
    reads, cands = _best_of_case(name)
    exp = _best_of_expected(name, mode)
    assert set(exp["best"].tolist()) >= {0, 2} and {cands[k][b][2] for k, b in enumerate(exp["best"])} == {0, 1}  # winners first and last, on both strands
    p = L.make_params(mode, MX, GO, GE)
    bo._check(bo._call(L, p, reads, None, cands, cigar=True, resident=True), exp, mode, True, "best of, %s" % name)
    assert L.get_timing()["fast_path"] == (8 if mode == 3 else 7)  # (the timing describes the score stage)
    bo._check(bo._call(L, p, reads, None, cands, cigar=False, resident=True), exp, mode, False, "best of, %s, no CIGAR stage" % name)
    assert L.get_timing()["fast_path"] == (8 if mode == 3 else 7)
    bo._check(bo._call(L, p, reads, main, cands, cigar=True), exp, mode, True, "best of, %s: the byte-window twin" % name)
    RAN.add((name, "best_of/mode%d" % mode))


@functools.lru_cache(maxsize=None)
def _best_pair_case(name):
    """mates 2k / 2k + 1: reads of windows k and k + 1 of the class, the second one from the other strand; two candidates each"""
    import test_best_pair_gpu as bp
    wins, rs = pr.windows(name), pr.reads(name)
    n = len(wins) // 2 * 2
    reads, cands = [], []
    for k in range(n):
        reads.append(bp._rc(rs[k]) if k % 2 else rs[k])
        other = wins[(k + 2) % n]
        cands.append([(other[0], other[1], k % 2), (wins[k][0], wins[k][1], k % 2)] if k % 4 < 2 else [(wins[k][0], wins[k][1], k % 2), (other[0], other[1], 1 - k % 2)])
    return reads, cands, bp._expected(MX, GO, GE, reads, pr.main_ref(), cands, 0, 400, 300)


@pytest.mark.parametrize("name", CAND_CLASSES)
def test_best_pair(gpu_lib, main, name):
    import test_best_pair_gpu as bp
    L = gpu_lib
    reads, cands, exp = _best_pair_case(name)
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, MX, GO, GE)
    bp._check(bp._call(L, p, reads, None, cands, 0, 400, 300, resident=True), exp, True, "best pair, %s" % name)
    assert L.get_timing()["fast_path"] == 10
    bp._check(bp._call(L, p, reads, main, cands, 0, 400, 300), exp, True, "best pair, %s: the byte-window twin" % name)
    RAN.add((name, "best_pair"))


# ---- summaries and MD ----------------------------------------------------------------------------------------------------------------------------
M, I, D = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _hand_made():
    """(windows, reads, routes) in the mapping mode (the window is alpha, D = a window-only column): an M run of 80 columns that starts at
    every residue mod 16 of the reference, in a clean stretch and across the N of flag word 2; CIGARs that end on the last base"""
    g = pr.main_ref()
    rng = np.random.default_rng(5)
    wins, routes = [], []
    for base in (5000, 8192 + 640):
        for r in range(16):
            wins.append((base + r, 86))
            routes.append([(3, D), (80, M), (3, D)])
            wins.append((base + r, 80))
            routes.append([(80, M)])
    n = pr.MAIN_LEN
    for l, route in ((80, [(80, M)]), (81, [(4, D), (70, M), (2, I), (7, M)]), (1, [(1, M)]), (64, [(60, M), (4, D)]), (65, [(1, D), (64, M)])):
        wins.append((n - l, l))
        routes.append(route)
    reads = []
    for (s, l), route in zip(wins, routes):
        w, at, rd = g[s:s + l], 0, []
        for run, o in route:
            if o == I:
                rd.extend(rng.integers(0, 4, size=run).tolist())
                continue
            if o == M:
                rd.extend(int(b) if b < 4 and rng.random() < 0.9 else int(rng.integers(0, 4)) for b in w[at:at + run])  # (a base against every N: its letter goes into MD)
            at += run
        reads.append(np.asarray(rd, np.uint8))
    return wins, reads, routes


@functools.lru_cache(maxsize=None)
def _cigar_case(name, mode):
    """(windows, reads, routes): the oracle's CIGARs of the class -- in the mapping mode the window is alpha"""
    if name == "hand_made":
        return _hand_made()
    wins, reads = pr.windows(name), pr.reads(name)
    g = pr.main_ref()
    res = oracle.align_batch(3, MX, GO, GE, _slices(g, wins), reads, threads=8) if mode == 3 else _align_expected(name, 1, mode)
    return wins, reads, _routes_of(res)


SUMMARY_CLASSES = pr.RUN_CLASSES + ("hand_made",)


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("name", SUMMARY_CLASSES)
def test_summary_and_md(gpu_lib, monkeypatch, main, name, form):
    import pyref_md
    import pyref_summary
    from gonomics_amd import align
    L = gpu_lib
    monkeypatch.setenv("GNX_SUMMARY_FORM", form)
    monkeypatch.setenv("GNX_MD_FORM", form)
    for mode in ((3,) if name == "hand_made" else (3, 0)):
        wins, reads, routes = _cigar_case(name, mode)
        ops, off = align._routes_to_ops(routes)
        cat, r_off = _cat(reads)
        ws, wl = _tables(wins)
        p = L.make_params(mode, MX, GO, GE)
        out, xops, xoff = L.summarize_batch_by_offset(p, cat, r_off, ws, wl, ops, off, xcigar=True)
        t = L.get_timing()
        assert t["fast_path"] == 12 and t["cells"] == sum(r for route in routes for r, _ in route)
        for k, route in enumerate(routes):
            w = main[wins[k][0]:wins[k][0] + wins[k][1]]
            a, b = (w, reads[k]) if mode == 3 else (reads[k], w)
            exp, ex = pyref_summary.summarize(mode, MX, GO, GE, a, b, route)
            assert {f: int(out[f][k]) for f in pyref_summary.FIELDS} == exp and int(out["_reserved"][k]) == 0, (name, mode, form, wins[k])
            assert [(int(r), int(o)) for r, o in zip(xops["run_length"][xoff[k]:xoff[k + 1]], xops["op"][xoff[k]:xoff[k + 1]])] == ex, (name, mode, form, wins[k])
        if mode == 3:
            twin = L.summarize_batch_windows(p, main, ws, wl, cat, r_off[:-1], np.diff(r_off), ops, off, xcigar=True)
        else:
            twin = L.summarize_batch_windows(p, cat, r_off[:-1], np.diff(r_off), main, ws, wl, ops, off, xcigar=True)
        assert twin[0].tobytes() == out.tobytes() and (twin[2] == xoff).all() and (twin[1]["op"] == xops["op"]).all() and (twin[1]["run_length"] == xops["run_length"]).all()
        if mode == 3:
            got = L.md_strings(*L.md_batch_by_offset(p, cat, r_off, ws, wl, ops, off))
            assert L.get_timing()["fast_path"] == 13
            want = [pyref_md.md(3, main[s:s + l], reads[k], routes[k]) for k, (s, l) in enumerate(wins)]
            wrong = [(wins[k], got[k][:60], want[k][:60]) for k in range(len(wins)) if got[k] != want[k]]
            assert not wrong, (name, form, wrong[:4])
            assert got == L.md_strings(*L.md_batch_windows(p, main, ws, wl, cat, r_off[:-1], np.diff(r_off), ops, off))
            if name in ("start_mod", "hand_made"):
                assert sum(t.count("N") for t in want) > 0  # the reference letters under N columns
    RAN.add((name, "summary/form" + form))
    RAN.add((name, "md/form" + form))


# ---- the pile --------------------------------------------------------------------------------------------------------------------------------------
PILE_REGIONS = [(0, pr.MAIN_LEN), (pr.MAIN_LEN - 70, 70), (4033, 128), (8192, 4096)]
PILE_CLASSES = ("start_mod", "end_mod", "beside_n", "all_n", "full_word", "to_the_end", "clean_edges")


@functools.lru_cache(maxsize=None)
def _pile_batch():
    """the reads of the classes with the oracle's CIGARs in the mapping mode, every other one from the reverse strand (the strand byte
    only: the reads are oriented as aligned), and qualities"""
    wins, reads, strands, routes = [], [], [], []
    for name in PILE_CLASSES:
        w, r, rt = _cigar_case(name, 3)
        wins += list(w); reads += list(r); routes += rt
    strands = [k % 2 for k in range(len(wins))]
    import test_pile_qual_gpu as tpq
    return wins, reads, strands, routes, tpq._quals(reads)


@functools.lru_cache(maxsize=None)
def _pile_expected(region, min_baseq):
    import pile_allele_cases as pac
    import pileup_cases as pc
    import pyref_pile_alleles as pa
    import pyref_pile_qual as pq
    import pyref_pileup as pp
    import test_pile_qual_gpu as tpq
    g = pr.main_ref()
    wins, reads, strands, routes, quals = _pile_batch()
    pile, alleles = pac.restate(g, region, wins, reads, strands, routes)
    qpile = tpq._restate(region, (wins, reads, strands, routes), quals, min_baseq)
    codes = g[region[0]:region[0] + region[1]]
    opts = pc.opts(min_depth=1, min_alt=1, frac=(1, 3))
    return {"pile": pile, "calls": pp.calls(pile, codes, opts, region_start=region[0]), "alleles": pa.listed(alleles),
            "indel_calls": pa.calls(alleles, pile, codes, opts, region_start=region[0]), "opts": opts,
            "qtables": tpq._tables(qpile), "genotypes": pq.genotypes(qpile, codes, pq.opts(2), region_start=region[0])}


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("region", PILE_REGIONS, ids=["%d_%d" % r for r in PILE_REGIONS])
def test_pile(gpu_lib, monkeypatch, main, region, form):
    import pyref_pile_qual as pq
    import test_pile_alleles_gpu as tpa
    import test_pile_qual_gpu as tpq
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    L = gpu_lib
    monkeypatch.setenv("GNX_PILE_FORM", form)
    wins, reads, strands, routes, quals = _pile_batch()
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, MX, GO, GE)
    want = _pile_expected(region, 0)
    rows = tpg._as_rows(want["pile"])
    o = want["opts"]
    # without qualities, tracking alleles
    tpa._open_tracking(*region)
    tpg._add(p, (wins, reads, strands, routes))
    assert L.get_timing()["fast_path"] == 14
    got = align.PileupGet()
    assert not tpg._differences(got, rows, region[0]), tpg._differences(got, rows, region[0])
    calls = L.pileup_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"])
    assert tpg._call_tuples(calls) == want["calls"] and L.get_timing()["fast_path"] == 15
    assert tpa._allele_tuples(L.pileup_alleles()) == want["alleles"]
    assert tpa._call_tuples(L.pileup_indel_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"])) == want["indel_calls"]
    # with qualities
    align.PileupOpen(*region)
    align.PileupTrackQualities(0)
    tpq._add(p, (wins, reads, strands, routes), quals)
    got, got_q = tpq._both()
    qrows, qsum = want["qtables"]
    assert not tpg._differences(got, qrows, region[0]) and not tpg._differences(qrows, rows, region[0])
    assert (got_q == qsum).all(), np.nonzero((got_q != qsum).any(axis=1))[0][:5]
    go = pq.opts(2)
    geno = L.pileup_genotypes(go["min_depth"], go["min_qual"], go["prior_het"], go["prior_hom"])
    assert tpq._geno_tuples(geno) == tpq._want_tuples(want["genotypes"]) and L.get_timing()["fast_path"] == 20
    if region[1] > 1000:
        assert len(want["calls"]) > 0 and int(rows["base"].sum()) > 1000
    RAN.add(("region_%d_%d" % region, "pile/form" + form))


@pytest.mark.parametrize("ln", [l for l in pr.ENDS_LENGTHS if 63 <= l <= 4097])
def test_pile_over_a_whole_reference(gpu_lib, ln):
    import pile_allele_cases as pac
    import pileup_cases as pc
    import pyref_pile_alleles as pa
    import pyref_pileup as pp
    import test_pile_alleles_gpu as tpa
    import test_pile_qual_gpu as tpq
    import test_pileup_gpu as tpg
    from gonomics_amd import align
    L = gpu_lib
    p = L.make_params(L.GNX_AFFINE_GAP_LOCAL, MX, GO, GE)
    try:
        for variant in pr.ENDS_VARIANTS:
            g = pr.ends_refs()[(ln, variant)]
            wins = [w for w in pr.ends_windows(ln) if w[1] <= 300] + [(max(0, ln - 150), min(ln, 150)), (0, min(ln, 64))]
            reads = [np.minimum(g[s:s + l], 4) for s, l in wins]
            if ln >= 63:  # one read that lacks two bases of its window and one that has three more: a deletion and an insertion near the end
                reads[-2] = np.concatenate([reads[-2][:-12], reads[-2][-10:]])
                reads[-1] = np.concatenate([reads[-1][:40], np.asarray([(int(reads[-1][40]) + 1) % 4] * 3, np.uint8), reads[-1][40:]])
            routes = _routes_of(oracle.align_batch(3, MX, GO, GE, _slices(g, wins), reads, threads=8))
            strands = [k % 2 for k in range(len(wins))]
            batch = (wins, reads, strands, routes)
            quals = tpq._quals(reads)
            L.set_reference(g)
            tpa._open_tracking(0, ln)
            tpg._add(p, batch)
            assert L.get_timing()["fast_path"] == 14
            pile, alleles = pac.restate(g, (0, ln), *batch)
            got = align.PileupGet()
            assert not tpg._differences(got, tpg._as_rows(pile), 0), (ln, variant)
            o = pc.opts(min_depth=1, min_alt=1, frac=(1, 3))
            calls = L.pileup_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"])
            assert L.get_timing()["fast_path"] == 15
            assert tpg._call_tuples(calls) == pp.calls(pile, g, o, region_start=0), (ln, variant)
            assert tpa._allele_tuples(L.pileup_alleles()) == pa.listed(alleles), (ln, variant)
            assert L.get_timing()["fast_path"] == 16
            align.PileupOpen(0, ln)
            align.PileupTrackQualities(0)
            tpq._add(p, batch, quals)
            assert L.get_timing()["fast_path"] == 14
            rows, qsum = tpq._tables(tpq._restate((0, ln), batch, quals, 0))
            got, got_q = tpq._both()
            assert not tpg._differences(got, rows, 0) and (got_q == qsum).all(), (ln, variant)
    finally:
        L.set_reference(np.zeros(0, np.uint8))
    RAN.add(("ends_%d" % ln, "pile"))


# ---- the pile's normalisation: repeats whose left end is a border -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _norm_case():
    """a copy of main with homopolymers and period-2 / period-3 repeats of 24 bases planted so that each one's left end is: base 0 of the
    reference (which takes the N there away), one base behind an N (65, 13 200, and 8 193, 10 208, 12 223, 12 288 behind the N of bits 0, 31,
    62, 63 of flag word 2), the flag-word border 4 096 (behind what stays of the N run there), every residue mod 32 (5 000 + 97 r, r = 0 ..
    31: 32 repeats of 24 bases do not fit one 64-base stretch), and one within 48 bases of the last base; a deletion and an
    insertion of one period at the RIGHT end of every repeat, which normalisation moves to the left end"""
    g = pr.main_ref().copy()
    rng = np.random.default_rng(77)
    behind_n = [(65, 2), (8193, 2), (8192 + 65 * 31 + 1, 1), (8192 + 65 * 62 + 1, 3), (12288, 2), (13200, 3)]  # (flag word 2: bits 0, 31, 62, 63)
    residues = [(5000 + 97 * r, 1 + r % 3) for r in range(32)]
    lefts = [(0, 1), (4096, 3), (pr.MAIN_LEN - 45, 2)] + behind_n + residues
    assert {left % 32 for left, _ in residues} == set(range(32)) and all(pr.main_ref()[left - 1] == 4 for left, _ in behind_n)
    wins, reads, strands, routes = [], [], [], []
    for left, period in lefts:
        span = 24 if left < pr.MAIN_LEN - 100 else 20
        unit = rng.permutation(4)[:period].astype(np.uint8)
        if left > 0 and g[left - 1] < 4:
            unit[-1] = (g[left - 1] + 1) % 4 if unit[-1] == g[left - 1] else unit[-1]  # the repeat begins here and not before
        g[left:left + span] = np.resize(unit, span)
        if left + span < len(g) and g[left + span] < 4:
            g[left + span] = (np.resize(unit, span + 1)[span] + 1) % 4  # ... and ends here
    for left, period in lefts:
        span = 24 if left < pr.MAIN_LEN - 100 else 20
        s = max(0, left - 8)
        e = min(len(g), left + span + 8)
        w = g[s:e]
        pre, post = left + span - period - s, e - (left + span)
        for kind in (D, I):
            if kind == D:  # the last period of the repeat is missing from the read
                rd = np.concatenate([w[:pre], w[pre + period:]])
                rt = [(pre, M), (period, D), (post, M)]
            else:          # one more period in the read
                rd = np.concatenate([w[:pre + period], w[pre:pre + period], w[pre + period:]])
                rt = [(pre + period, M), (period, I), (post, M)]
            wins.append((s, e - s)); reads.append(np.minimum(rd, 4).astype(np.uint8)); strands.append(len(wins) % 2); routes.append([x for x in rt if x[0] > 0])
    return g, lefts, (wins, reads, strands, routes)


@pytest.mark.parametrize("coop", ["0", "1"])
@pytest.mark.parametrize("region", [(0, pr.MAIN_LEN), (4096, 4200), (5000, 3300)], ids=["whole", "from_4096", "from_5000"])
def test_pile_normalisation(gpu_lib, monkeypatch, region, coop):
    import pile_allele_cases as pac
    import pileup_cases as pc
    import pyref_pile_alleles as pa
    import pyref_pile_norm as pn
    import test_pile_alleles_gpu as tpa
    import test_pileup_gpu as tpg
    L = gpu_lib
    monkeypatch.setenv("GNX_NORM_COOP", coop)
    g, lefts, batch = _norm_case()
    wins, reads, strands, routes = batch
    pile, alleles = pac.restate(g, region, wins, reads, strands, routes)
    plain = pa.listed(alleles)
    codes = g[region[0]:region[0] + region[1]]
    moved_alleles = pn.normalized(alleles, g.tolist(), region)
    moved = pa.listed(moved_alleles)
    inside = [(left, per) for left, per in lefts if region[0] <= left and left + 24 <= region[0] + region[1]]
    assert moved != plain and len(inside) >= 5
    if region[0] in (4096, 5000):
        assert any(left == region[0] for left, _ in inside)  # a repeat whose left end is the first base of the region
    L.set_reference(g)
    try:
        tpa._open_tracking(*region)
        tpg._add(L.make_params(L.GNX_AFFINE_GAP_LOCAL, MX, GO, GE), batch)
        assert tpa._allele_tuples(L.pileup_alleles(normalize=True)) == moved
        assert L.get_timing()["fast_path"] == 18
        assert tpa._allele_tuples(L.pileup_alleles()) == plain
        o = pc.opts(min_depth=1, min_alt=1, frac=(1, 3))
        want = pa.calls(moved_alleles, pile, codes, o, region_start=region[0])
        assert tpa._call_tuples(L.pileup_indel_calls(o["min_depth"], o["min_alt"], o["frac_num"], o["frac_den"], o["both_strands"], normalize=True)) == want
    finally:
        L.set_reference(np.zeros(0, np.uint8))
    RAN.add(("region_%d_%d" % region, "pile_norm/coop" + coop))


# ---- the index and the seed candidates -------------------------------------------------------------------------------------------------------------
KS = (8, 16, 32)
STEPS = (1, 7)


def _check_index(L, g, k, step, what):
    L.reference_index_build(k, step)
    keys, pos = L.reference_index_get()
    table = pyref_seeds.index(g, k, step)
    assert keys.tolist() == [c for c, _ in table] and pos.tolist() == [q for _, q in table], what
    assert L.reference_index_info()["n_kmers"] == len(table)
    return {q for _, q in table}


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("k", KS)
def test_index_of_main(gpu_lib, main, k, step):
    present = _check_index(gpu_lib, main, k, step, (k, step))
    if step == 1:  # what the equality says, spelled out on the borders
        n = len(main)
        assert (n - k in present) == bool((main[n - k:] < 4).all()) and n - k not in present  # the last k-mer holds the N at the last base
        for lo, hi in pr.stretches(main):
            if lo - k >= 0 and (main[lo - k:lo] < 4).all():
                assert lo - k in present                     # ends one base before the stretch
            assert lo - k + 1 not in present or lo - k + 1 < 0  # ends on its first base
            assert hi - 1 not in present                     # starts on its last base
            if hi + k <= n and (main[hi:hi + k] < 4).all():
                assert hi in present                         # starts one base behind it
        assert 12288 in present and 12288 - k not in present  # a block border where only the first block is flagged ...
        assert 4090 - k in present and (8192 - k in present) and 8192 - k + 1 not in present  # ... and one where only the second is
        inside = [q for q in present if 8192 <= q < 12288 - k]
        assert len(inside) == sum(1 for q in range(8192, 12288 - k) if (main[q:q + k] < 4).all()) > 0  # inside flag word 2
    RAN.add(("main", "index/k%d/step%d" % (k, step)))


@pytest.mark.parametrize("ln", pr.ENDS_LENGTHS)
def test_index_of_ends(gpu_lib, ln):
    L = gpu_lib
    try:
        for variant in pr.ENDS_VARIANTS:
            g = pr.ends_refs()[(ln, variant)]
            L.set_reference(g)
            for k in KS:
                for step in STEPS:
                    present = _check_index(L, g, k, step, (ln, variant, k, step))  # (a reference shorter than k: an empty index)
                    if step == 1 and ln >= k:
                        assert (ln - k in present) == (variant == "clean")
                    assert ln >= k or not present
    finally:
        L.set_reference(np.zeros(0, np.uint8))
    RAN.add(("ends_%d" % ln, "index"))


@pytest.mark.parametrize("k", [16, 32])
def test_seed_candidates(gpu_lib, main, k):
    import test_best_of_gpu as bo
    L = gpu_lib
    reads = []
    for name in ("to_the_end", "beside_n"):
        for j, (s, l) in enumerate(pr.windows(name)):
            r = np.minimum(main[s:s + l], 4)
            reads.append(bo._rc(r) if j % 2 else r.copy())
    opts = dict(max_occ=16, bin=32, pad=16, max_cand=4, min_votes=1)
    L.reference_index_build(k, 1)
    cat, off = _cat(reads)
    c_off, st, ln, sd, votes = L.seed_candidates(cat[:-1] if len(cat) > 1 else cat, off, **opts)
    assert L.get_timing()["fast_path"] == 11
    exp = pyref_seeds.candidates_batch(main, k, 1, reads, **opts)
    got = [[(int(st[c]), int(ln[c]), int(sd[c]), int(votes[c])) for c in range(c_off[r], c_off[r + 1])] for r in range(len(reads))]
    assert got == exp
    assert any(c[2] == 1 for cs in exp for c in cs) and any(c[0] + c[1] == len(main) for cs in exp for c in cs)  # the other strand; a candidate that ends with the reference
    RAN.add(("to_the_end+beside_n", "seed_candidates/k%d" % k))


# ---- errors: a window that touches a byte >= 5 --------------------------------------------------------------------------------------------------------
GUARD = 0xA5
SENTINEL_PTR = 0x5A5A  # an output pointer that a refused call must leave as it was


def _guarded(n, dtype):
    a = np.zeros(max(n, 1), dtype=dtype)
    a.view(np.uint8)[:] = GUARD
    return a


def _untouched(*arrays):
    return all((a.view(np.uint8) == GUARD).all() for a in arrays)


def test_bad_bytes(gpu_lib, main):
    """every entry that takes windows: GNX_EBASE, the outputs untouched, and the next clean call gives the oracle's result"""
    import ctypes
    import pyref_span
    from gonomics_amd import align
    L = gpu_lib
    lib = L.lib()
    bad, ok = pr.windows("bad_bytes"), pr.windows("bad_bytes_ok")
    rng = np.random.default_rng(3)
    ok_reads = [common.mutate(rng, main[s + 10:s + 110], alphabet=4) for s, l in ok]
    ok_cat, ok_off = _cat(ok_reads)
    ok_s, ok_l = _tables(ok)
    ok_exp = oracle.align_batch(0, MX, GO, GE, ok_reads, _slices(main, ok), threads=2)
    ok_spans = pyref_span.spans_from_oracle(MX, GO, GE, _slices(main, ok), ok_reads, threads=2)
    pg, pl = L.make_params(0, MX, GO, GE), L.make_params(3, MX, GO, GE)
    for s, l in bad:
        # a batch of three: clean, bad, clean -- one bad window fails the call
        wins = [ok[0], (s, l), ok[1]]
        rd = np.minimum(main[s:s + min(l, 100)], 3)
        reads = [ok_reads[0], rd, ok_reads[1]]
        cat, off = _cat(reads)
        ws, wl = _tables(wins)
        n = 3
        sc, en, st = _guarded(n, np.int64), _guarded(n, np.int64), _guarded(n, np.int64)
        ops_p, off_p = ctypes.c_void_p(SENTINEL_PTR), ctypes.c_void_p(SENTINEL_PTR)
        args = (n, cat.ctypes.data, off.ctypes.data, ws.ctypes.data, wl.ctypes.data)
        assert lib.gnx_align_batch_by_offset(ctypes.byref(pg), *args, sc.ctypes.data, ctypes.byref(ops_p), ctypes.byref(off_p)) == L.GNX_EBASE, (s, l)
        assert _untouched(sc) and ops_p.value == SENTINEL_PTR and off_p.value == SENTINEL_PTR
        for p in (pg, pl):
            assert lib.gnx_score_batch_by_offset(ctypes.byref(p), *args, sc.ctypes.data) == L.GNX_EBASE, (s, l)
            assert _untouched(sc)
        assert lib.gnx_locate_batch_by_offset(ctypes.byref(pl), *args, sc.ctypes.data, en.ctypes.data) == L.GNX_EBASE
        assert lib.gnx_locate_span_batch_by_offset(ctypes.byref(pl), *args, sc.ctypes.data, st.ctypes.data, en.ctypes.data) == L.GNX_EBASE
        assert _untouched(sc, en, st)
        # best of, best pair: the bad window as a losing candidate
        cands = [[ok[0] + (0,), (s, l, 0)], [(s, l, 1)], [ok[1] + (0,)], [ok[1] + (1,)]]
        four = reads + [ok_reads[1]]
        assert _raw_best_of(L, pg, four, cands) == (L.GNX_EBASE, True), (s, l)
        assert _raw_best_of(L, pl, four, cands) == (L.GNX_EBASE, True), (s, l)
        assert _raw_best_pair(L, pl, four, cands) == (L.GNX_EBASE, True), (s, l)
        # summary, MD, pile: a CIGAR of M columns over the window
        routes = [[(len(r), M), (w[1] - len(r), D)] if w[1] > len(r) else [(w[1], M), (len(r) - w[1], I)] for r, w in zip(reads, wins)]
        routes = [[x for x in rt if x[0] > 0] for rt in routes]
        ops, o_off = align._routes_to_ops(routes)
        out = _guarded(n, L.SUMMARY_DTYPE)
        with pytest.raises(L.GnxError) as ei:
            L.summarize_batch_by_offset(pl, cat, off, ws, wl, ops, o_off, out=out)
        assert ei.value.code == L.GNX_EBASE and _untouched(out), (s, l)
        md_p, mdoff_p = ctypes.c_void_p(SENTINEL_PTR), ctypes.c_void_p(SENTINEL_PTR)
        raw_ops, raw_off = L._ops_array(ops), np.ascontiguousarray(o_off, np.int64)
        assert lib.gnx_md_batch_by_offset(ctypes.byref(pl), *args, raw_ops.ctypes.data, raw_off.ctypes.data, ctypes.byref(md_p), ctypes.byref(mdoff_p)) == L.GNX_EBASE, (s, l)
        assert md_p.value == SENTINEL_PTR and mdoff_p.value == SENTINEL_PTR
        xp, xo = ctypes.c_void_p(SENTINEL_PTR), ctypes.c_void_p(SENTINEL_PTR)
        assert lib.gnx_summarize_batch_by_offset(ctypes.byref(pl), *args, raw_ops.ctypes.data, raw_off.ctypes.data, out.ctypes.data, ctypes.byref(xp), ctypes.byref(xo)) == L.GNX_EBASE
        assert _untouched(out) and xp.value == SENTINEL_PTR and xo.value == SENTINEL_PTR
        align.PileupOpen(0, len(main))
        L.pileup_add_by_offset(pl, ok_cat, ok_off, ok_s, ok_l, [0, 1], *align._routes_to_ops([[(len(r), M), (w[1] - len(r), D)] for r, w in zip(ok_reads, ok)]))
        before = align.PileupGet().tobytes()
        with pytest.raises(L.GnxError) as ei:
            L.pileup_add_by_offset(pl, cat, off, ws, wl, [0, 1, 0], ops, o_off)
        assert ei.value.code == L.GNX_EBASE and align.PileupGet().tobytes() == before and align.PileupInfo()["reads_added"] == 2, (s, l)
        # the next clean call
        common.assert_same(L.align_batch_by_offset(pg, ok_cat, ok_off, ok_s, ok_l), ok_exp, "after GNX_EBASE")
    assert np.array_equal(L.score_batch_by_offset(pg, ok_cat, ok_off, ok_s, ok_l), ok_exp[0])
    got = L.locate_span_batch_by_offset(pl, ok_cat, ok_off, ok_s, ok_l)
    assert all(np.array_equal(a, b) for a, b in zip(got, ok_spans))
    assert np.array_equal(L.score_batch_by_offset(pl, ok_cat, ok_off, ok_s, ok_l), oracle.align_batch(3, MX, GO, GE, ok_reads, _slices(main, ok))[0])
    RAN.add(("bad_bytes", "errors"))


def _cand_tables(reads, cands):
    r_cat, r_off = _cat(reads)
    c_off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
    flat = [c for cs in cands for c in cs]
    return (r_cat, r_off, c_off, np.asarray([c[0] for c in flat], np.int64), np.asarray([c[1] for c in flat], np.int64), np.asarray([c[2] for c in flat], np.uint8))


def _raw_best_of(L, p, reads, cands):
    """gnx_best_of_by_offset itself on guarded outputs: (return code, nothing written)"""
    import ctypes
    r_cat, r_off, c_off, st, ln, sd = _cand_tables(reads, cands)
    n, nc = len(reads), len(st)
    best, score, end, cand = _guarded(n, np.int32), _guarded(n, np.int64), _guarded(n, np.int64), _guarded(nc, np.int64)
    ops, off = ctypes.c_void_p(SENTINEL_PTR), ctypes.c_void_p(SENTINEL_PTR)
    rc = L.lib().gnx_best_of_by_offset(ctypes.byref(p), n, r_cat.ctypes.data, r_off.ctypes.data, c_off.ctypes.data, st.ctypes.data, ln.ctypes.data, sd.ctypes.data,
                                       best.ctypes.data, score.ctypes.data, end.ctypes.data if p.mode == L.GNX_AFFINE_GAP_LOCAL else None, cand.ctypes.data,
                                       ctypes.byref(ops), ctypes.byref(off))
    return rc, _untouched(best, score, end, cand) and ops.value == SENTINEL_PTR and off.value == SENTINEL_PTR


def _raw_best_pair(L, p, reads, cands):
    """gnx_best_pair_by_offset itself on guarded outputs: (return code, nothing written)"""
    import ctypes
    r_cat, r_off, c_off, st, ln, sd = _cand_tables(reads, cands)
    n, nc = len(reads), len(st)
    o = L.pair_opts(0, 400, 300)
    outs = [_guarded(n, np.int32)] + [_guarded(n, np.int64) for _ in range(4)] + [_guarded(n // 2, np.uint8), _guarded(n // 2, np.int64)] + [_guarded(nc, np.int64) for _ in range(3)]
    ops, off = ctypes.c_void_p(SENTINEL_PTR), ctypes.c_void_p(SENTINEL_PTR)
    rc = L.lib().gnx_best_pair_by_offset(ctypes.byref(p), ctypes.byref(o), n, r_cat.ctypes.data, r_off.ctypes.data, c_off.ctypes.data, st.ctypes.data, ln.ctypes.data, sd.ctypes.data,
                                         *[a.ctypes.data for a in outs], ctypes.byref(ops), ctypes.byref(off))
    return rc, _untouched(*outs) and ops.value == SENTINEL_PTR and off.value == SENTINEL_PTR


# ---- two contexts ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_contexts(gpu_lib, monkeypatch):
    """both contexts hold the reference (ensure_reference's copy, sized by ref_words / ref_flagwords) and read it alike: the read-back, align
    and score on main and on the lengths whose one-past look-ups land in the padding words; a reference set while two contexts exist,
    then replaced by a shorter one"""
    L = gpu_lib
    lib = L.lib()
    monkeypatch.setenv("GNX_RCCL", "0")
    lib.gnx_shutdown()
    try:
        assert L.init_devices([0, 0]) == 2
        g = pr.main_ref()
        L.set_reference(g)  # set while two contexts exist
        pos = np.asarray([s for s, _ in pr.windows("every_base")], np.int64)
        _read_back(L, monkeypatch, pos, g[pos], "main, two contexts", two_contexts=True)
        p = L.make_params(0, MX, GO, GE)
        for name in ("start_mod", "beside_n", "to_the_end", "full_word"):
            reads, wins = pr.reads(name), pr.windows(name)
            rep = (16 + len(wins) - 1) // len(wins)  # batches of 16 pairs and more: both contexts get a share
            cat, off = _cat(reads * rep)
            ws, wl = _tables(wins * rep)
            exp = _align_expected(name, 1, 0)
            for env in ({}, FAST):
                with monkeypatch.context() as mp:
                    _apply(mp, env)
                    sc, ops, o = L.align_batch_by_offset(p, cat, off, ws, wl)
                    tm = L.get_timing()
                    assert tm["n_contexts"] == 2, name
                    _route_is(tm, 1 if env else _default_route(name), (name, env, "two contexts"))
                k = len(wins)
                for r in range(rep):
                    assert np.array_equal(sc[r * k:(r + 1) * k], exp[0]), (name, env)
                    a, b = o[r * k], o[(r + 1) * k]
                    assert np.array_equal(o[r * k:(r + 1) * k + 1] - a, exp[2]) and np.array_equal(ops["run_length"][a:b], exp[1]["run_length"]) and np.array_equal(ops["op"][a:b], exp[1]["op"]), (name, env)
            sc = L.score_batch_by_offset(p, cat, off, ws, wl)
            tm = L.get_timing()
            assert tm["n_contexts"] == 2 and tm["fast_path"] == 7 and np.array_equal(sc, np.tile(exp[0], rep)), name
            RAN.add((name, "two_contexts"))
        for ln in (8192, 4096, 4095):  # each one shorter than the one before: replaced in place on both contexts
            for variant in pr.ENDS_VARIANTS:
                h = pr.ends_refs()[(ln, variant)]
                L.set_reference(h)
                assert L.reference_info()[0] == ln and L.reference_info()[2] == pr.flagged_blocks(h)
                _read_back(L, monkeypatch, np.arange(ln), h, ("two contexts", ln, variant), two_contexts=True)
                _ends_every_entry(L, monkeypatch, ln, variant, rep=6, contexts=2)  # 18 pairs: both contexts get a share
            RAN.add(("ends_%d" % ln, "two_contexts"))
    finally:
        lib.gnx_shutdown()
        L.check(lib.gnx_init(0, 0))


# ---- nothing was skipped ----------------------------------------------------------------------------------------------------------------------------------
def expected_table():
    t = {("every_base", "read_back"), ("synthetic", "read_back"), ("bad_bytes", "errors")}
    t |= {("ends_%d" % ln, what) for ln in pr.ENDS_LENGTHS for what in ("read_back", "windows", "index")}
    t |= {("ends_%d" % ln, "pile") for ln in pr.ENDS_LENGTHS if 63 <= ln <= 4097}
    t |= {("ends_%d" % ln, "two_contexts") for ln in (4095, 4096, 8192)}
    for name in pr.RUN_CLASSES:
        t |= {(name, "align/" + how) for how in ALIGN_ROUTES} | {(name, "score"), (name, "locate"), (name, "span")}
    for name in SUMMARY_CLASSES:
        t |= {(name, "%s/form%s" % (e, f)) for e in ("summary", "md") for f in "01"}
    for name in CAND_CLASSES:
        t |= {(name, "best_of/mode0"), (name, "best_of/mode3"), (name, "best_pair")}
    t |= {("region_%d_%d" % r, "pile/form" + f) for r in PILE_REGIONS for f in "01"}
    t |= {("region_%d_%d" % r, "pile_norm/coop" + c) for r in ((0, pr.MAIN_LEN), (4096, 4200), (5000, 3300)) for c in "01"}
    t |= {("main", "index/k%d/step%d" % (k, s)) for k in KS for s in STEPS} | {("to_the_end+beside_n", "seed_candidates/k%d" % k) for k in (16, 32)}
    t |= {(name, "two_contexts") for name in ("start_mod", "beside_n", "to_the_end", "full_word")}
    return t


def _items_of_the_module():
    """the number of test items this module has when nothing is deselected, from the parametrisations themselves"""
    n = 0
    for name, fn in globals().items():
        if name.startswith("test_") and callable(fn):
            k = 1
            for mark in getattr(fn, "pytestmark", []):
                if mark.name == "parametrize":
                    k *= len(mark.args[1])
            n += k
    return n


def test_every_class_ran(request):
    """no class and no entry was skipped: the (class, entry) cells that ran are cells of the table -- all of them, when the whole module
    was selected"""
    table = expected_table()
    assert RAN <= table, sorted(RAN - table)
    assert len(table) >= 210 and len(pr.RUN_CLASSES) == 7 and len(ALIGN_ROUTES) == 11
    selected = [it for it in request.session.items if it.module.__name__ == __name__]
    if len(selected) == _items_of_the_module():
        assert RAN == table, sorted(table - RAN)[:10]
