"""Score-only entries on the device (gnx_score_*): every comparison is exact equality of int64 scores with the score of
oracle.align_batch(...) -- no tolerance, no case left out -- and with the score of the align call on the same library."""
import numpy as np
import pytest

import common
import oracle
from gonomics_amd import align

pytestmark = pytest.mark.gpu
MX = common.matrices()
GLOBAL_MODES = (0, 1, 2, 4)


def _params(L, mode, mx, go, ge):
    return L.make_params(mode, mx, go, ge if mode in (0, 2, 3) else 0)


def _check_lists(L, mode, mx, go, ge, alphas, betas, route=None, threads=8, what=""):
    """score call == oracle == align call for a batch given as lists; returns the timing of the score call"""
    p = _params(L, mode, mx, go, ge)
    got = L.score_batch(p, alphas, betas)
    tm = L.get_timing()
    exp = oracle.align_batch(mode, mx, go, ge if mode in (0, 2, 3) else 0, alphas, betas, threads=threads)[0]
    assert got.dtype == np.int64 and np.array_equal(got, exp), (what, mode, np.flatnonzero(got != exp)[:8], got[:4], exp[:4])
    assert np.array_equal(got, L.align_batch(p, alphas, betas)[0]), what
    if route is True:
        assert tm["fast_path"] == 7, (what, tm["fast_path"])
    elif route is False:
        assert tm["fast_path"] != 7, what
    return tm


@pytest.mark.parametrize("mode", range(5))
@pytest.mark.parametrize("mname", sorted(MX))
def test_fuzz_all_modes(gpu_lib, mode, mname):
    """random_pairs with N bases, n, m in 1 .. 400 including n > m, n == 1, m == 1 (and empty sequences in the high-memory modes)"""
    go, ge = (-400, -30) if mode in (0, 2, 3) else (-430, 0)
    alphas, betas = common.random_pairs(500 + mode, 260, 1, 400, 1, 400)
    one = np.zeros(1, dtype=np.uint8)
    alphas += [one, np.asarray([3], np.uint8), alphas[0], one]
    betas += [betas[1], np.asarray([3], np.uint8), one, one + 2]
    _check_lists(gpu_lib, mode, MX[mname], go, ge, alphas, betas, route=(mode != 3), what="fuzz " + mname)
    if mode in (2, 3, 4):  # the high-memory modes take empty sequences
        e = np.zeros(0, dtype=np.uint8)
        _check_lists(gpu_lib, mode, MX[mname], go, ge, alphas[:40] + [e, alphas[3], e], betas[:40] + [betas[2], e, e], route=False, what="empty " + mname)


@pytest.mark.parametrize("mode", (0, 1))
def test_error_codes_match_the_align_call(gpu_lib, mode):
    p = _params(gpu_lib, mode, MX["Default"], -400, -30)
    a, b = common.random_pairs(9, 6, 5, 50, 5, 50)
    for alphas, betas, code in ((a + [np.zeros(0, np.uint8)], b + [b[0]], gpu_lib.GNX_EEMPTY), (a + [np.asarray([0, 1, 7, 2], np.uint8)], b + [b[0]], gpu_lib.GNX_EBASE),
                                (a + [a[0]], b + [np.asarray([0, 5], np.uint8)], gpu_lib.GNX_EBASE)):
        codes = []
        for fn in (gpu_lib.align_batch, gpu_lib.score_batch):
            with pytest.raises(gpu_lib.GnxError) as ei:
                fn(p, alphas, betas)
            codes.append(ei.value.code)
        assert codes == [code, code]
    with pytest.raises(IndexError):
        align.AffineGapScore(np.asarray([0, 9], np.uint8), np.asarray([0, 1], np.uint8), MX["Default"], -400, -30)
    with pytest.raises(ValueError):
        align.ConstGapScore(np.zeros(0, np.uint8), np.asarray([0, 1], np.uint8), MX["Default"], -400)


@pytest.mark.parametrize("mode", GLOBAL_MODES)
@pytest.mark.parametrize("go,ge", [(0, -30), (-400, 0), (0, 0), (-7, -3)])
def test_ties_and_degenerate_penalties(gpu_lib, mode, go, ge):
    rng = np.random.default_rng(11)
    alphas = [np.full(n, b, np.uint8) for n, b in ((1, 0), (17, 0), (160, 2), (161, 2), (333, 3), (40, 4))]
    betas = [np.full(m, b, np.uint8) for m, b in ((9, 0), (400, 0), (150, 2), (500, 2), (320, 0), (77, 4))]
    alphas += [rng.integers(0, 2, size=n).astype(np.uint8) for n in (50, 200, 321)]
    betas += [rng.integers(0, 2, size=m).astype(np.uint8) for m in (300, 190, 322)]
    flat = [[1, -1, -1, -1, 0]] * 4 + [[0, 0, 0, 0, 0]]
    for mx in (MX["Default"], flat):
        _check_lists(gpu_lib, mode, mx, go, ge, alphas, betas, route=True, what="ties %d %d" % (go, ge))


def _c2_mixed(seed, n_pairs, chunk_len=10000):
    """C2 shape with reads of 1 .. 160 and of 161 .. 700 bases in one batch (one, two and several row blocks)"""
    reads, chunk = common.c2_workload(seed, n_pairs, read_len=700, chunk_len=chunk_len)
    rng = np.random.default_rng(seed + 1)
    a_len = np.where(rng.random(n_pairs) < 0.5, rng.integers(1, 161, size=n_pairs), rng.integers(161, 701, size=n_pairs)).astype(np.int64)
    a_len[:4] = (1, 160, 161, 700)
    a_start = np.arange(n_pairs, dtype=np.int64) * 700
    b_start = np.zeros(n_pairs, dtype=np.int64)
    b_len = np.full(n_pairs, chunk_len, dtype=np.int64)
    return reads.reshape(-1), a_start, a_len, chunk, b_start, b_len


@pytest.mark.parametrize("mode", (0, 1))
def test_c2_shape_windows_and_resident_reference(gpu_lib, mode):
    mx, go, ge = MX["HumanChimpTwo"], -600, (-150 if mode == 0 else 0)
    a, a_start, a_len, chunk, b_start, b_len = _c2_mixed(21 + mode, 2400)
    chunk = chunk.copy()
    chunk[4096:4096 + 200] = 4  # an N block: windows that touch it read the exception list of the packed reference
    p = _params(gpu_lib, mode, mx, go, ge)
    exp = oracle.align_batch_windows(mode, mx, go, ge, a, a_start, a_len, chunk, b_start, b_len, threads=16)[0]
    got = gpu_lib.score_batch_windows(p, a, a_start, a_len, chunk, b_start, b_len)
    assert gpu_lib.get_timing()["fast_path"] == 7
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]
    assert np.array_equal(got, gpu_lib.align_batch_windows(p, a, a_start, a_len, chunk, b_start, b_len)[0])
    # the resident reference (packed 2 bit), windows of several lengths, some on the N block, some shorter than their read (n > m)
    rng = np.random.default_rng(5)
    n = 600
    lens = a_len[:n]
    cat = np.concatenate([a[s:s + l] for s, l in zip(a_start[:n], lens)])
    a_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r_len = rng.integers(1, 3000, size=n).astype(np.int64)
    r_start = rng.integers(0, chunk.shape[0] - 3000, size=n).astype(np.int64)
    r_start[::7] = 4000
    gpu_lib.set_reference(chunk)
    try:
        got = gpu_lib.score_batch_by_offset(p, cat, a_off, r_start, r_len)
        assert gpu_lib.get_timing()["fast_path"] == 7
        exp = oracle.align_batch_windows(mode, mx, go, ge, cat, a_off[:-1], lens, chunk, r_start, r_len, threads=16)[0]
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8]
        assert np.array_equal(got, gpu_lib.align_batch_by_offset(p, cat, a_off, r_start, r_len)[0])
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))


@pytest.mark.parametrize("mode", (0, 1))
def test_general_shape_both_orientations(gpu_lib, mode):
    """a few dozen pairs with both sides 2 000 .. 10 000, n > m and n < m"""
    alphas, betas = common.random_pairs(31 + mode, 28, 2000, 10000, 2000, 10000, with_n=False)
    alphas += [betas[0], alphas[1][:10000], alphas[2][:2000]]
    betas += [alphas[0], betas[1][:2000], betas[2][:10000]]
    assert any(len(a) > len(b) for a, b in zip(alphas, betas)) and any(len(a) < len(b) for a, b in zip(alphas, betas))
    _check_lists(gpu_lib, mode, MX["HumanChimpTwo"], -600, -150, alphas, betas, route=True, threads=16, what="general shape")


def test_fallback_routes(gpu_lib):
    rng = np.random.default_rng(41)
    a, b = common.random_pairs(42, 24, 1, 300, 1, 300)
    _check_lists(gpu_lib, 3, MX["Default"], -400, -30, a, b, route=False, what="local")
    for mode in GLOBAL_MODES:
        _check_lists(gpu_lib, mode, MX["Default"], 25, -30, a, b, route=False, what="gapOpen > 0")
    long_a, long_b = rng.integers(0, 4, size=30000).astype(np.uint8), rng.integers(0, 4, size=12000).astype(np.uint8)
    _check_lists(gpu_lib, 0, MX["Default"], -400, -30, [long_a, a[0]], [long_b, b[0]], route=False, threads=16, what="past the sweep's length limit")
    big = (np.asarray(MX["Default"], dtype=np.int64) * 100000).tolist()  # the static bound (n + m + 2) * max|penalty| leaves int32 at a few hundred bases
    _check_lists(gpu_lib, 2, big, -400 * 100000, -30 * 100000, a, b, route=False, what="beyond int32")
    _check_lists(gpu_lib, 4, big, -400 * 100000, 0, a, b, route=False, what="beyond int32, constant gap")


def test_score_equals_align_on_100k_c2_pairs(gpu_lib):
    reads, chunk = common.c2_workload(51, 1000)
    n = 100000
    a_start = (np.arange(n, dtype=np.int64) % 1000) * 150
    a_len = np.full(n, 150, dtype=np.int64)
    rng = np.random.default_rng(52)
    b_len = rng.integers(9000, 10001, size=n).astype(np.int64)
    b_start = rng.integers(0, 10000 - b_len + 1).astype(np.int64)
    for mode, ge in ((0, -150), (1, 0)):
        p = _params(gpu_lib, mode, MX["HumanChimpTwo"], -600, ge)
        got = gpu_lib.score_batch_windows(p, reads.reshape(-1), a_start, a_len, chunk, b_start, b_len)
        assert gpu_lib.get_timing()["fast_path"] == 7
        assert np.array_equal(got, gpu_lib.align_batch_windows(p, reads.reshape(-1), a_start, a_len, chunk, b_start, b_len)[0])


def test_score_all_pairs_and_one_pair_functions(gpu_lib):
    rng = np.random.default_rng(61)
    root = rng.integers(0, 4, size=900).astype(np.uint8)
    seqs = [common.mutate(rng, root, sub=0.05, indel=0.02) for _ in range(12)]
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, MX["Default"], -400, -30)
    got = align.ScoreAllPairs(seqs, p)
    assert sorted(got) == [(x, y) for x in range(12) for y in range(x + 1, 12)]
    for (x, y), s in got.items():
        assert s == oracle.align_one(0, MX["Default"], -400, -30, seqs[x], seqs[y])[0], (x, y)
    a, b = seqs[0], seqs[1][:300]
    assert align.AffineGapScore(a, b, MX["Default"], -400, -30) == align.AffineGap(a, b, MX["Default"], -400, -30)[0] == oracle.align_one(0, MX["Default"], -400, -30, a, b)[0]
    assert align.ConstGapScore(a, b, MX["Default"], -430) == align.ConstGap(a, b, MX["Default"], -430)[0] == oracle.align_one(1, MX["Default"], -430, 0, a, b)[0]
    assert align.AffineGapLocalScore(a, b, MX["Default"], -400, -30) == align.AffineGapLocal(a, b, MX["Default"], -400, -30)[0] == oracle.align_one(3, MX["Default"], -400, -30, a, b)[0]


def test_align_best_of(gpu_lib):
    """500 reads x 8 candidate windows each (one of them the read's origin): index, score and route equal "oracle on all pairs, first maximum\""""
    R, K, W = 500, 8, 400
    rng = np.random.default_rng(71)
    ref = rng.integers(0, 4, size=60000).astype(np.uint8)
    reads, wins = [], []
    for r in range(R):
        o = int(rng.integers(0, ref.shape[0] - W))
        reads.append(common.mutate(rng, ref[o + 100:o + 250], sub=0.02, indel=0.01)[:150])
        ws = [(int(x), W) for x in rng.integers(0, ref.shape[0] - W, size=K)]
        ws[int(rng.integers(0, K))] = (o, W)
        if r % 50 == 0:
            ws[5] = ws[2]  # an exact tie: the first one wins
        wins.append(ws)
    mx, go, ge = MX["HumanChimpTwo"], -600, -150
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, mx, go, ge)
    exp_s, exp_ops, exp_off = oracle.align_batch(0, mx, go, ge, [reads[r] for r in range(R) for _ in range(K)], [ref[s:s + l] for ws in wins for s, l in ws], threads=16)
    want = [int(np.argmax(exp_s[r * K:(r + 1) * K])) for r in range(R)]  # (argmax: the first maximum)
    by_seq = align.AlignBestOf(p, reads, [[ref[s:s + l] for s, l in ws] for ws in wins])
    gpu_lib.set_reference(ref)
    try:
        by_win = align.AlignBestOf(p, reads, wins)
    finally:
        gpu_lib.set_reference(np.zeros(0, np.uint8))
    for got in (by_seq, by_win):
        for r, (b, s, route) in enumerate(got):
            k = r * K + want[r]
            assert b == want[r] and s == int(exp_s[k]), r
            assert route == [align.Cigar(int(x), int(o)) for x, o in zip(exp_ops["run_length"][exp_off[k]:exp_off[k + 1]], exp_ops["op"][exp_off[k]:exp_off[k + 1]])], r


def test_two_contexts_on_one_device(gpu_lib, monkeypatch):
    L = gpu_lib.lib()
    a, a_start, a_len, chunk, b_start, b_len = _c2_mixed(81, 1200, chunk_len=3000)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, MX["HumanChimpTwo"], -600, -150)
    one = gpu_lib.score_batch_windows(p, a, a_start, a_len, chunk, b_start, b_len)
    assert np.array_equal(one, oracle.align_batch_windows(0, MX["HumanChimpTwo"], -600, -150, a, a_start, a_len, chunk, b_start, b_len, threads=16)[0])
    alphas, betas = common.random_pairs(82, 240, 1, 500, 1, 900)
    pl = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, MX["Default"], -400, -30)
    one_l = gpu_lib.score_batch(pl, alphas, betas)
    try:
        gpu_lib.check(L.gnx_shutdown() or 0)
        monkeypatch.setenv("GNX_RCCL", "0")
        assert gpu_lib.init_devices([0, 0], 8 << 30) == 2
        two = gpu_lib.score_batch_windows(p, a, a_start, a_len, chunk, b_start, b_len)
        tm = gpu_lib.get_timing()
        assert np.array_equal(two, one)
        assert tm["n_contexts"] == 2 and tm["transport"] == 2 and tm["fast_path"] == 7
        assert np.array_equal(gpu_lib.score_batch(pl, alphas, betas), one_l)  # a fallback route, sharded
        assert gpu_lib.get_timing()["fast_path"] != 7
    finally:
        monkeypatch.delenv("GNX_RCCL", raising=False)
        L.gnx_shutdown()
        gpu_lib.check(L.gnx_init(0, 8 << 30))
