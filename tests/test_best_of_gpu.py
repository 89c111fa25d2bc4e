"""Best-of-K read placement on both strands (gnx_best_of_windows / gnx_best_of_by_offset, align.MapBestOf).
Expected values come from the CPU oracle on the FLATTENED pair list -- the reverse complement taken on the host, the first maximum
found in Python -- and every comparison is exact equality: candidate scores, winners, winners' scores and CIGARs, target ends."""
import ctypes

import numpy as np
import pytest

import common
import oracle
from gonomics_amd import align

pytestmark = pytest.mark.gpu
MX = common.matrices()
FLAT = [[1, -1, -1, -1, 0]] * 4 + [[0, 0, 0, 0, 0]]
AFFINE, CONST, HIGHMEM, LOCAL = 0, 1, 2, 3
PEN = {AFFINE: (-400, -30), CONST: (-430, 0), HIGHMEM: (-400, -30), LOCAL: (-400, -30)}


def _rc(x):
    """host restatement of the device's reverse complement: reversed, A <-> T, C <-> G, everything else unchanged"""
    x = np.asarray(x, np.uint8)[::-1].copy()
    m = x < 4
    x[m] = 3 - x[m]
    return x


def _flatten(mode, reads, target, cands):
    """the pair list the contract speaks of: global modes alpha = read', beta = window; local: alpha (target) = window, beta (query) = read'"""
    alphas, betas = [], []
    for rd, cs in zip(reads, cands):
        for s, l, st in cs:
            r2, w = (_rc(rd) if st else np.asarray(rd, np.uint8)), np.asarray(target[s:s + l], np.uint8)
            alphas.append(w if mode == LOCAL else r2)
            betas.append(r2 if mode == LOCAL else w)
    return alphas, betas


def _first_max(v):
    b = 0
    for k in range(1, len(v)):
        if v[k] > v[b]:
            b = k
    return b


def _expected(mode, mx, go, ge, reads, target, cands, ci=10000, cj=10000):
    alphas, betas = _flatten(mode, reads, target, cands)
    if alphas:
        sc, ops, off = oracle.align_batch(mode, mx, go, ge, alphas, betas, ci, cj, threads=16)
    else:
        sc, ops, off = np.zeros(0, np.int64), np.zeros(0, oracle.CIGAR_DTYPE), np.zeros(1, np.int64)
    n = len(reads)
    exp = {"cand": np.asarray(sc, np.int64), "best": np.full(n, -1, np.int32), "score": np.zeros(n, np.int64), "end": np.zeros(n, np.int64), "routes": [[] for _ in range(n)]}
    at = 0
    for r, cs in enumerate(cands):
        if cs:
            b = _first_max(sc[at:at + len(cs)])
            w = at + b
            exp["best"][r], exp["score"][r] = b, sc[w]
            exp["routes"][r] = [(int(x), int(o)) for x, o in zip(ops["run_length"][off[w]:off[w + 1]], ops["op"][off[w]:off[w + 1]])]
            end = len(alphas[w])  # local: the target length minus the trailing ColD run
            if exp["routes"][r] and exp["routes"][r][-1][1] == 2:
                end -= exp["routes"][r][-1][0]
            exp["end"][r] = end
        at += len(cs)
    return exp


def _tables(reads, cands):
    r_cat = np.concatenate([np.asarray(r, np.uint8) for r in reads] + [np.zeros(1, np.uint8)])
    r_off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    c_off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
    flat = [c for cs in cands for c in cs]
    return r_cat, r_off, c_off, [c[0] for c in flat], [c[1] for c in flat], [c[2] for c in flat]


def _call(L, p, reads, target, cands, cigar=True, resident=False):
    r_cat, r_off, c_off, st, ln, sd = _tables(reads, cands)
    if resident:
        return L.best_of_by_offset(p, r_cat, r_off, c_off, st, ln, sd, cigar=cigar)
    return L.best_of_windows(p, r_cat, r_off, target, c_off, st, ln, sd, cigar=cigar)


def _check(got, exp, mode, cigar, what=""):
    best, score, ends, cand, ops, off = got
    assert best.dtype == np.int32 and score.dtype == np.int64 and cand.dtype == np.int64
    assert np.array_equal(cand, exp["cand"]), (what, "candidate scores", np.flatnonzero(cand != exp["cand"])[:8])
    assert np.array_equal(best, exp["best"]), (what, "best", np.flatnonzero(best != exp["best"])[:8])
    assert np.array_equal(score, exp["score"]), (what, "score", np.flatnonzero(score != exp["score"])[:8])
    if mode == LOCAL:
        assert np.array_equal(ends, exp["end"]), (what, "end", np.flatnonzero(ends != exp["end"])[:8])
    else:
        assert ends is None
    if not cigar:
        assert ops is None and off is None
        return
    assert off.shape[0] == len(exp["routes"]) + 1 and off[0] == 0
    for r, route in enumerate(exp["routes"]):
        mine = [(int(x), int(o)) for x, o in zip(ops["run_length"][off[r]:off[r + 1]], ops["op"][off[r]:off[r + 1]])]
        assert mine == route, (what, "route of read", r, mine[:6], route[:6])


def _workload(seed, n_reads, kmax=5, target_len=12000, short=(1, 40), long=(120, 200), wmax=600, kmin=0):
    """reads are mutated pieces of the target, half of them from the other strand; K candidates per read, about half of the reads with
    one candidate over their origin on the right strand, the rest at random places and strands"""
    rng = np.random.default_rng(seed)
    target = rng.integers(0, 4, size=target_len).astype(np.uint8)
    target[rng.random(target_len) < 0.01] = 4
    reads, cands = [], []
    for r in range(n_reads):
        lo, hi = short if r % 2 else long
        ln = int(rng.integers(lo, hi + 1))
        o = int(rng.integers(0, target_len - ln))
        rd = common.mutate(rng, target[o:o + ln], sub=0.04, indel=0.02, geo=0.4, alphabet=5)
        if len(rd) == 0:
            rd = target[o:o + 1].copy()
        strand = int(rng.integers(0, 2))
        reads.append(_rc(rd) if strand else np.asarray(rd, np.uint8))
        cs = []
        for k in range(int(rng.integers(kmin, kmax + 1))):
            wl = int(rng.integers(1, wmax + 1))
            if k == 1 or (k == 0 and rng.random() < 0.3):
                s = max(0, o - int(rng.integers(0, 150)))
                cs.append((s, min(max(wl, ln + 100), wmax, target_len - s), strand))
            else:
                cs.append((int(rng.integers(0, target_len - wl)), wl, int(rng.integers(0, 2))))
        cands.append(cs)
    return reads, target, cands


_FUZZ = {}


def _fuzz_workload():
    if not _FUZZ:
        _FUZZ["w"] = _workload(101, 200)
    return _FUZZ["w"]


@pytest.mark.parametrize("mname", sorted(MX))
@pytest.mark.parametrize("mode", [AFFINE, CONST, HIGHMEM, LOCAL])
def test_fuzz(gpu_lib, mode, mname):
    """200 reads of 1 .. 40 and 120 .. 200 bases, 0 .. 5 windows of 1 .. 600 bases each, random strands; with and without the CIGAR
    stage; the low-memory modes once with the default checkerboard and once with a small one"""
    reads, target, cands = _fuzz_workload()
    assert any(len(c) == 0 for c in cands) and any(len(c) == 5 for c in cands)
    go, ge = PEN[mode]
    ck = 37 if mname in ("HumanChimpTwo", "MouseRat") else 10000
    p = gpu_lib.make_params(mode, MX[mname], go, ge, ck, ck)
    exp = _expected(mode, MX[mname], go, ge, reads, target, cands, ck, ck)
    flat_strands = [c[2] for cs in cands for c in cs]
    assert 0 < sum(flat_strands) < len(flat_strands)
    assert any(cs[b][2] == 1 for cs, b in zip(cands, exp["best"]) if cs) and any(b > 0 for b in exp["best"])
    _check(_call(gpu_lib, p, reads, target, cands, cigar=True), exp, mode, True, "fuzz")
    _check(_call(gpu_lib, p, reads, target, cands, cigar=False), exp, mode, False, "fuzz, no CIGAR stage")


@pytest.mark.parametrize("mode", [AFFINE, CONST, HIGHMEM, LOCAL])
def test_ties_go_to_the_first_candidate(gpu_lib, mode):
    rng = np.random.default_rng(7)
    go, ge = PEN[mode]
    mx = MX["Default"]
    p = gpu_lib.make_params(mode, mx, go, ge)
    # duplicated windows: candidates 0 == 1 and 2 == 3
    target = rng.integers(0, 4, size=3000).astype(np.uint8)
    reads, cands = [], []
    for r in range(30):
        o, ln = int(rng.integers(0, 2500)), int(rng.integers(20, 180))
        reads.append(common.mutate(rng, target[o:o + ln]))
        a, b = (o, min(400, 3000 - o), 0), (int(rng.integers(0, 2500)), 300, 1)
        cands.append([a, a, b, b] if r % 2 else [b, b, a, a])
    exp = _expected(mode, mx, go, ge, reads, target, cands)
    assert set(exp["best"].tolist()) == {0, 2}
    _check(_call(gpu_lib, p, reads, target, cands), exp, mode, True, "duplicated windows")
    # reads that equal their own reverse complement, offered on both strands of one window, in either order
    pal = [align.dna.StringToBases(s) for s in ("ACGT", "AATT", "ACGTACGT", "GAATTC", "AACGTT", "TA")]
    for s in pal:
        assert np.array_equal(_rc(s), s)
    win = np.concatenate([target[:40], pal[2], target[40:80]])
    reads, cands = pal + pal, [[(10, 70, 0), (10, 70, 1)]] * len(pal) + [[(10, 70, 1), (10, 70, 0)]] * len(pal)
    exp = _expected(mode, mx, go, ge, reads, win, cands)
    got = _call(gpu_lib, p, reads, win, cands)
    _check(got, exp, mode, True, "palindromes")
    assert np.all(got[0] == 0) and np.array_equal(got[3][0::2], got[3][1::2])


@pytest.mark.parametrize("go,ge", [(0, -30), (-400, 0), (0, 0)])
def test_two_letter_sequences_with_degenerate_penalties(gpu_lib, go, ge):
    rng = np.random.default_rng(13)
    target = rng.integers(0, 2, size=4000).astype(np.uint8)
    reads = [rng.integers(0, 2, size=int(n)).astype(np.uint8) for n in rng.integers(1, 200, size=40)]
    reads += [np.full(n, b, np.uint8) for n, b in ((9, 0), (160, 0), (161, 3), (50, 1))]  # (3: T, the complement of the letter A)
    cands = [[(int(rng.integers(0, 3500)), int(rng.integers(1, 400)), int(rng.integers(0, 2))) for _ in range(4)] for _ in reads]
    for mx in (MX["Default"], FLAT):
        for mode in (AFFINE, LOCAL, CONST):
            g, e = (go, 0) if mode == CONST else (go, ge)
            exp = _expected(mode, mx, g, e, reads, target, cands)
            _check(_call(gpu_lib, gpu_lib.make_params(mode, mx, g, e), reads, target, cands), exp, mode, True, "two letters %d %d mode %d" % (go, ge, mode))


@pytest.mark.parametrize("mode", [AFFINE, LOCAL])
def test_block_edges_and_transposition(gpu_lib, mode):
    """reads around one, two and three row blocks of the score sweep against windows of 700 (the one-block and the levels kernels), and
    reads of 300 against windows of 100 (the window in the lanes, the reverse-complemented read streaming as columns)"""
    rng = np.random.default_rng(19)
    target = rng.integers(0, 5, size=5000).astype(np.uint8)
    reads, cands = [], []
    for ln, wl in [(159, 700), (160, 700), (161, 700), (320, 700), (321, 700), (300, 100), (300, 100)] * 2:
        o = int(rng.integers(0, 4000))
        rd = common.mutate(rng, target[o:o + ln], sub=0.05, indel=0.03, geo=0.4, alphabet=5)
        rd = np.concatenate([rd, rng.integers(0, 4, size=ln).astype(np.uint8)])[:ln]
        strand = len(reads) % 2
        reads.append(_rc(rd) if strand else rd)
        cands.append([(int(rng.integers(0, 4200)), wl, 1 - strand), (max(0, min(o - 50, 5000 - wl)), wl, strand), (int(rng.integers(0, 4200)), wl, strand)])
    mx, (go, ge) = MX["HumanChimpTwo"], (-600, -150)
    p = gpu_lib.make_params(mode, mx, go, ge)
    exp = _expected(mode, mx, go, ge, reads, target, cands)
    for cigar in (True, False):
        _check(_call(gpu_lib, p, reads, target, cands, cigar=cigar), exp, mode, cigar, "block edges")
        tm = gpu_lib.get_timing()
        assert tm["fast_path"] == (8 if mode == LOCAL else 7), tm
        assert tm["cells"] == sum(len(r) * c[1] for r, cs in zip(reads, cands) for c in cs)
        assert tm["n_contexts"] == 1 and tm["host_ms"] > 0 and tm["total_ms"] > 0


def _raw_by_offset(L, p, reads, cands):
    """the C entry itself with sentinel-filled outputs: (return code, outputs untouched?)"""
    r_cat, r_off, c_off, st, ln, sd = _tables(reads, cands)
    st, ln, sd = np.asarray(st, np.int64), np.asarray(ln, np.int64), np.asarray(sd, np.uint8)
    n = len(reads)
    best, score, end, cand = np.full(n, 77, np.int32), np.full(n, 77, np.int64), np.full(n, 77, np.int64), np.full(len(st), 77, np.int64)
    ops, off = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.lib().gnx_best_of_by_offset(ctypes.byref(p), n, r_cat.ctypes.data, r_off.ctypes.data, c_off.ctypes.data, st.ctypes.data, ln.ctypes.data, sd.ctypes.data,
                                       best.ctypes.data, score.ctypes.data, end.ctypes.data if p.mode == LOCAL else None, cand.ctypes.data, ctypes.byref(ops), ctypes.byref(off))
    clean = bool(np.all(best == 77) and np.all(score == 77) and np.all(end == 77) and np.all(cand == 77) and not ops.value and not off.value)
    if rc == 0:
        L.lib().gnx_free(ops)
        L.lib().gnx_free(off)
    return rc, clean


def test_resident_reference(gpu_lib):
    """windows of the packed reference: over an N run they take the packed path (fast_path 7 / 8); a byte >= 5 matters only when a
    window touches it -- then, even for a losing candidate, the whole call is GNX_EBASE and nothing is written"""
    rng = np.random.default_rng(31)
    ref = rng.integers(0, 4, size=9000).astype(np.uint8)
    ref[3000:3300] = 4
    ref[7000] = 6
    reads, cands = [], []
    for r in range(48):
        ln = int(rng.integers(100, 200))
        o = int(rng.integers(2800, 3400 - ln)) if r % 3 == 0 else int(rng.integers(0, 6000))
        rd = common.mutate(rng, ref[o:o + ln], sub=0.03, indel=0.02, alphabet=5)
        strand = r % 2
        reads.append(_rc(rd) if strand else rd)
        cands.append([(int(rng.integers(0, 6300)), int(rng.integers(1, 600)), int(rng.integers(0, 2))), (max(0, o - 60), 400, strand), (2900, 500, strand)][:1 + r % 3])
    assert all(s + l <= 7000 for cs in cands for s, l, _ in cs)
    mx, (go, ge) = MX["HumanChimpTwo"], (-600, -150)
    clean = ref.copy()
    clean[7000] = 0  # (no window touches it: the same pairs for the entries that take the buffer as bytes)
    gpu_lib.set_reference(ref)
    try:
        for mode in (AFFINE, LOCAL):
            p = gpu_lib.make_params(mode, mx, go, ge)
            exp = _expected(mode, mx, go, ge, reads, ref, cands)
            got = _call(gpu_lib, p, reads, None, cands, resident=True)
            assert gpu_lib.get_timing()["fast_path"] == (8 if mode == LOCAL else 7)
            _check(got, exp, mode, True, "resident reference, mode %d" % mode)
            _check(_call(gpu_lib, p, reads, None, cands, cigar=False, resident=True), exp, mode, False, "resident reference, no CIGAR stage")
            _check(_call(gpu_lib, p, reads, clean, cands), exp, mode, True, "the same windows from a buffer")
            if mode == LOCAL:  # the twins themselves on the winners: align_batch_windows(alpha = window bytes, beta = read'), the locate twin on the packed reference
                win = [cs[b] for cs, b in zip(cands, got[0])]
                qs = [_rc(rd) if w[2] else rd for rd, w in zip(reads, win)]
                q_cat = np.concatenate(qs)
                q_off = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
                ws, wl = np.asarray([w[0] for w in win], np.int64), np.asarray([w[1] for w in win], np.int64)
                t_sc, t_ops, t_off = gpu_lib.align_batch_windows(p, clean, ws, wl, q_cat, q_off[:-1], np.diff(q_off))
                assert np.array_equal(got[1], t_sc) and np.array_equal(got[5], t_off)
                assert np.array_equal(got[4]["run_length"], t_ops["run_length"]) and np.array_equal(got[4]["op"], t_ops["op"])
                l_sc, l_end = gpu_lib.locate_batch_by_offset(p, q_cat, q_off, ws, wl)
                assert np.array_equal(got[1], l_sc) and np.array_equal(got[2], l_end)
            bad = [list(cs) for cs in cands]
            bad[5].append((6998, 3, 0))  # three bases against a read of >= 100: it cannot win, and it touches the byte 6
            assert _raw_by_offset(gpu_lib, p, reads, bad) == (gpu_lib.GNX_EBASE, True)
            bad_reads = [r.copy() for r in reads]
            bad_reads[7][3] = 9
            assert _raw_by_offset(gpu_lib, p, bad_reads, cands) == (gpu_lib.GNX_EBASE, True)
            assert _raw_by_offset(gpu_lib, p, reads, cands) == (gpu_lib.GNX_OK, False)
            outside = [list(cs) for cs in cands]
            outside[2].append((8990, 11, 0))
            assert _raw_by_offset(gpu_lib, p, reads, outside) == (gpu_lib.GNX_EINVAL, True)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    assert _raw_by_offset(gpu_lib, gpu_lib.make_params(AFFINE, mx, go, ge), reads, cands) == (gpu_lib.GNX_EINVAL, True)  # no resident reference


def test_fallback_routes(gpu_lib, monkeypatch):
    """gapOpen > 0 and GNX_SCORE_SWEEP=0: the score stage takes the align route, the results stay what they are"""
    reads, target, cands = _workload(47, 60, kmax=4)
    mx = MX["Default"]
    for mode in (AFFINE, LOCAL):
        p = gpu_lib.make_params(mode, mx, 25, -30)
        exp = _expected(mode, mx, 25, -30, reads, target, cands)
        _check(_call(gpu_lib, p, reads, target, cands), exp, mode, True, "gapOpen > 0")
        assert gpu_lib.get_timing()["fast_path"] not in (7, 8)
    for mode in (AFFINE, CONST, LOCAL):
        go, ge = PEN[mode]
        p = gpu_lib.make_params(mode, mx, go, ge)
        exp = _expected(mode, mx, go, ge, reads, target, cands)
        monkeypatch.delenv("GNX_SCORE_SWEEP", raising=False)
        _check(_call(gpu_lib, p, reads, target, cands), exp, mode, True, "the sweep")
        assert gpu_lib.get_timing()["fast_path"] == (8 if mode == LOCAL else 7)
        monkeypatch.setenv("GNX_SCORE_SWEEP", "0")
        for cigar in (True, False):
            _check(_call(gpu_lib, p, reads, target, cands, cigar=cigar), exp, mode, cigar, "GNX_SCORE_SWEEP=0")
            assert gpu_lib.get_timing()["fast_path"] not in (7, 8)
    # the same switch on the packed reference (local mode: the fallback unpacks the candidates' windows)
    gpu_lib.set_reference(target)
    try:
        for mode in (AFFINE, LOCAL):
            go, ge = PEN[mode]
            exp = _expected(mode, mx, go, ge, reads, target, cands)
            _check(_call(gpu_lib, gpu_lib.make_params(mode, mx, go, ge), reads, None, cands, resident=True), exp, mode, True, "GNX_SCORE_SWEEP=0, resident")
            assert gpu_lib.get_timing()["fast_path"] not in (7, 8)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


def _twin_code(L, mode, p, alphas, betas):
    try:
        (L.locate_batch if mode == LOCAL else L.score_batch)(p, alphas, betas)
    except L.GnxError as e:
        return e.code
    return L.GNX_OK


@pytest.mark.parametrize("mode", [AFFINE, CONST, HIGHMEM, LOCAL])
def test_degenerate_inputs(gpu_lib, mode):
    rng = np.random.default_rng(5)
    go, ge = PEN[mode]
    mx = MX["Default"]
    p = gpu_lib.make_params(mode, mx, go, ge)
    target = rng.integers(0, 4, size=800).astype(np.uint8)
    reads = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (30, 150, 7)]
    # no candidates at all, no reads at all
    for cigar in (True, False):
        best, score, ends, cand, ops, off = _call(gpu_lib, p, reads, target, [[], [], []], cigar=cigar)
        assert best.tolist() == [-1, -1, -1] and score.tolist() == [0, 0, 0] and cand.shape == (0,)
        assert ends is None or ends.tolist() == [0, 0, 0]
        assert (off.tolist() == [0, 0, 0, 0] and ops.shape == (0,)) if cigar else off is None
        best, score, ends, cand, ops, off = _call(gpu_lib, p, [], target, [], cigar=cigar)
        assert best.shape == (0,) and score.shape == (0,) and (off.tolist() == [0] if cigar else off is None)
    # reads without candidates between reads that have some
    cands = [[], [(100, 300, 1), (0, 200, 0)], []]
    _check(_call(gpu_lib, p, reads, target, cands), _expected(mode, mx, go, ge, reads, target, cands), mode, True, "reads without candidates")
    # an empty read, an empty window: the twin's code (GNX_EEMPTY in the low-memory modes), else the twin's results
    empty = np.zeros(0, np.uint8)
    for what, rs, cs in (("empty read", [reads[0], empty, reads[2]], [[(0, 100, 0)], [(5, 50, 0), (9, 60, 1)], [(300, 40, 1)]]),
                         ("empty window", reads, [[(0, 100, 0)], [(5, 50, 0), (9, 0, 1)], [(300, 40, 1)]])):
        code = _twin_code(gpu_lib, mode, p, *_flatten(mode, rs, target, cs))
        assert code == (gpu_lib.GNX_EEMPTY if mode in (AFFINE, CONST) else gpu_lib.GNX_OK), (what, code)
        if code:
            for cigar in (True, False):
                with pytest.raises(gpu_lib.GnxError) as ei:
                    _call(gpu_lib, p, rs, target, cs, cigar=cigar)
                assert ei.value.code == code, what
        else:
            _check(_call(gpu_lib, p, rs, target, cs), _expected(mode, mx, go, ge, rs, target, cs), mode, True, what)


@pytest.mark.parametrize("sub", [104, 24])
def test_sub_batches(gpu_lib, monkeypatch, sub):
    """300 candidates in sub-batches of 104 (3 of them; 104 is no multiple of 5, so a read's candidates straddle each cut) and of 24
    (13 in the score stage, 3 in the CIGAR stage)"""
    reads, target, cands = _workload(59, 60, kmax=5, kmin=5)
    assert sum(len(c) for c in cands) == 300
    monkeypatch.setenv("GNX_HOST_SUB", str(sub))
    for mode in (AFFINE, LOCAL):
        go, ge = PEN[mode]
        exp = _expected(mode, MX["HumanChimpTwo"], go, ge, reads, target, cands)
        p = gpu_lib.make_params(mode, MX["HumanChimpTwo"], go, ge)
        _check(_call(gpu_lib, p, reads, target, cands), exp, mode, True, "sub-batches of %d" % sub)
        assert gpu_lib.get_timing()["n_launches"] == (3 if sub == 104 else 13)  # (one sweep per sub-batch of the score stage)
        gpu_lib.set_reference(target)
        try:
            _check(_call(gpu_lib, p, reads, None, cands, resident=True), exp, mode, True, "sub-batches of %d, resident" % sub)
        finally:
            gpu_lib.set_reference(np.zeros(0, np.uint8))


def test_two_contexts_on_one_device(gpu_lib, monkeypatch):
    L = gpu_lib.lib()
    reads, target, cands = _workload(83, 80, kmax=4)
    res = {}
    for mode in (AFFINE, LOCAL):
        go, ge = PEN[mode]
        exp = _expected(mode, MX["Default"], go, ge, reads, target, cands)
        res[mode] = (gpu_lib.make_params(mode, MX["Default"], go, ge), exp)
        _check(_call(gpu_lib, res[mode][0], reads, target, cands), exp, mode, True, "one context")
    try:
        gpu_lib.check(L.gnx_shutdown() or 0)
        monkeypatch.setenv("GNX_RCCL", "0")
        assert gpu_lib.init_devices([0, 0], 8 << 30) == 2
        for mode in (AFFINE, LOCAL):
            _check(_call(gpu_lib, res[mode][0], reads, target, cands), res[mode][1], mode, True, "two contexts")
            assert gpu_lib.get_timing()["fast_path"] == (8 if mode == LOCAL else 7)
            gpu_lib.set_reference(target)
            _check(_call(gpu_lib, res[mode][0], reads, None, cands, resident=True), res[mode][1], mode, True, "two contexts, resident")
            gpu_lib.set_reference(np.zeros(0, np.uint8))
    finally:
        monkeypatch.delenv("GNX_RCCL", raising=False)
        L.gnx_shutdown()
        gpu_lib.check(L.gnx_init(0, 8 << 30))


def test_python_map_best_of(gpu_lib):
    reads, target, cands = _workload(91, 24, kmax=3)
    mx = MX["Default"]
    for mode in (AFFINE, LOCAL):
        go, ge = PEN[mode]
        p = gpu_lib.make_params(mode, mx, go, ge)
        exp = _expected(mode, mx, go, ge, reads, target, cands)
        as_bases = [[(target[s:s + l], st) for s, l, st in cs] for cs in cands]
        gpu_lib.set_reference(target)
        try:
            outs = [align.MapBestOf(p, reads, cands), align.MapBestOf(p, reads, as_bases)]
            bare = align.MapBestOf(p, reads, cands, cigar=False)
        finally:
            gpu_lib.set_reference(np.zeros(0, np.uint8))
        at = 0
        for r, cs in enumerate(cands):
            want = (int(exp["best"][r]), int(exp["score"][r]), [align.Cigar(x, o) for x, o in exp["routes"][r]], int(exp["end"][r]) if mode == LOCAL else None,
                    [int(x) for x in exp["cand"][at:at + len(cs)]])
            for out in outs:
                assert out[r] == want, (mode, r, out[r], want)
            assert bare[r] == want[:2] + (None,) + want[3:]
            at += len(cs)
    assert align.MapBestOf(gpu_lib.make_params(AFFINE, mx, -400, -30), [], []) == []
    with pytest.raises(IndexError):
        align.MapBestOf(gpu_lib.make_params(AFFINE, mx, -400, -30), [np.asarray([0, 7, 1], np.uint8)], [[(target[:30], 1)]])
