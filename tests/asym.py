"""Helpers of the asymmetric-matrix tests (tests/test_asym_cpu.py, tests/test_asym_gpu.py).

Every score matrix the other suites use is symmetric, invariant under complementing both bases, and has an N row equal to its N
column, so a kernel or a host routine that transposes the table where it should not (or forgets to, or complements the table instead
of the read) passes them all.  ASYM is a table on which each of these mistakes changes the score of nearly every pair; the batches
below are the inputs of the GPU tests, kept here so that the CPU suite can check -- on the oracle alone -- that every one of them
really tells the orientations apart (assert_tells_orientation), and so that each expected result is computed once."""
import functools

import numpy as np

import common
import oracle

ASYM = [[91, -114, -31, -123, -44],
        [-101, 100, -125, -52, -37],
        [-58, -139, 97, -110, -49],
        [-133, -23, -96, 88, -61],
        [-40, -55, -29, -66, -43]]
COMPLEMENT = [3, 2, 1, 0, 4]  # A <-> T, C <-> G, N stays
ASYM_T = [[ASYM[b][a] for b in range(5)] for a in range(5)]
ASYM_RC = [[ASYM[COMPLEMENT[a]][COMPLEMENT[b]] for b in range(5)] for a in range(5)]
MATRICES = {"ASYM": ASYM, "ASYM_T": ASYM_T, "ASYM_RC": ASYM_RC}

AFFINE_PENS = [(-400, -30), (-600, -150)]
CONST_GAP = -430
GSW_GAP = -600
AFFINE_MODES = (0, 2, 3)


def pens(mode):
    """the penalty sets a mode is run with: both affine sets, or the one constant gap"""
    return AFFINE_PENS if mode in AFFINE_MODES else [(CONST_GAP, 0)]


def rc(x):
    """reverse complement: reversed, A <-> T, C <-> G, everything else unchanged"""
    x = np.asarray(x, np.uint8)[::-1].copy()
    m = x < 4
    x[m] = 3 - x[m]
    return x


# ---- the condition that keeps a batch from passing vacuously ------------------------------------------------------------------------
def _oracle_scores(mode, mx, go, ge, alphas, betas, ci, cj, threads):
    """(scores, full oracle result) of a batch; mode: 0 .. 4 (oracle.align_batch), ("chunk", c) (AffineGapChunk), ("multi", c)
    (multipleAffineGap on alignment blocks), ("gsw", side) (Left / RightDynamicAln, go = the gap penalty)"""
    if isinstance(mode, tuple):
        kind, arg = mode
        if kind == "chunk":
            res = [oracle.affine_gap_chunk(mx, go, ge, arg, a, b) for a, b in zip(alphas, betas)]
        elif kind == "multi":
            res = [oracle.multiple_affine_gap(mx, go, ge, arg, a, b) for a, b in zip(alphas, betas)]
        elif kind == "gsw":
            res = [oracle.gsw_extend(arg, mx, go, a, b) for a, b in zip(alphas, betas)]
        else:
            raise ValueError(kind)
        return np.asarray([r[0] for r in res], dtype=np.int64), res
    res = oracle.align_batch(mode, mx, go, ge, alphas, betas, ci, cj, threads=threads)
    return np.asarray(res[0], dtype=np.int64), res


def assert_tells_orientation(mode, go, ge, alphas, betas, other=ASYM_T, min_frac=0.5, ci=10000, cj=10000, threads=8):
    """Runs the oracle under ASYM and under `other` (ASYM_T: a transposed table, ASYM_RC: a complemented one) and fails unless the
    scores differ for at least min_frac of the pairs: a batch on which they do not could not show a wrong orientation.  A condition
    on the INPUTS, not a tolerance.  Returns what the oracle gave under ASYM."""
    mine, res = _oracle_scores(mode, ASYM, go, ge, alphas, betas, ci, cj, threads)
    theirs, _ = _oracle_scores(mode, other, go, ge, alphas, betas, ci, cj, threads)
    assert len(mine) > 0
    frac = float(np.mean(mine != theirs))
    assert frac >= min_frac, "only %.2f of %d pairs tell ASYM from the other table (mode %r, %d %d)" % (frac, len(mine), mode, go, ge)
    return res


# ---- the batches -------------------------------------------------------------------------------------------------------------------
def _ragged(seed, count, nmax, mmax):
    from test_const_long import _ragged as ragged
    return ragged(seed, count, nmax, mmax)


def _related(seed, shapes):
    """pairs (n rows, `extra` more columns) of related sequences, as tests/test_long_range.py builds them"""
    from test_long_range import _related as related
    rng = np.random.default_rng(seed)
    alphas, betas = [], []
    for n, extra, sub, indel in shapes:
        a, b = related(rng, n, extra, sub=sub, indel=indel)
        alphas.append(a); betas.append(b)
    return rng, alphas, betas


def _reads_in_windows(seed, count, n_lo, n_hi, ref_len=4000, m_choice=(128, 129, 255, 256, 257, 300, 1000, 1500, 2049)):
    """reads of n_lo .. n_hi bases (6 % substitutions, 2 % indels) cut from windows of one reference with a few N: the read at the
    window's start, at its end, or in the middle; one read in seven unrelated; windows shorter than the read among them"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=ref_len, dtype=np.uint8)
    ref[rng.integers(0, ref_len, size=8)] = 4
    edge = [n_lo, n_hi, min(n_lo + 1, n_hi), max(n_hi - 1, n_lo)]
    reads, wins = [], []
    for k in range(count):
        n = edge[k] if k < 4 else int(rng.integers(n_lo, n_hi + 1))
        m = int(rng.choice(m_choice))
        off = int(rng.integers(0, ref_len - m + 1))
        win = ref[off:off + m].copy()
        where = k % 4
        pos = 0 if where == 0 else (max(0, m - n) if where == 1 else int(rng.integers(0, max(1, m - n + 1))))
        if m >= n and k % 7 != 6:
            read = common.mutate(rng, win[pos:pos + n + 20], 0.06, 0.02)[:n]
        else:
            read = rng.integers(0, 4, size=n, dtype=np.uint8)
        if read.shape[0] < n_lo:  # (mutate may have shortened it)
            read = np.concatenate([read, rng.integers(0, 4, size=n_lo - read.shape[0], dtype=np.uint8)])
        reads.append(np.ascontiguousarray(read, dtype=np.uint8)); wins.append(win)
    return reads, wins


def _cheap_gap_reads(seed, count=48, chunk_len=1500):
    """tests/test_gpu_parity.py's overflow shape: every sixth read is every OTHER base of a piece of the chunk -- with gaps as cheap as
    (-30, -10) its CIGAR alternates M and I for more runs than the fast path stages.  Such an alignment has no mismatch left (a gap
    pair is cheaper), and neither has a read that may spread over a long window, so these pairs cannot tell a table from its
    transpose; the other reads get windows a few bases longer than themselves, where substitutions stay substitutions."""
    rng = np.random.default_rng(seed)
    chunk = rng.integers(0, 4, size=chunk_len).astype(np.uint8)
    reads, wins = [], []
    for k in range(count):
        off = int(rng.integers(10, chunk_len - 300))
        if k % 6 == 3:
            reads.append(chunk[off:off + 280:2][:140].copy()); wins.append(chunk)
        else:
            reads.append(common.mutate(rng, chunk[off:off + 150], 0.06, 0.005)[:150])
            wins.append(chunk[off - int(rng.integers(0, 8)):off + 150 + int(rng.integers(0, 8))].copy())
    return reads, wins


CHEAP_GAPS = (-30, -10)


def _similar_lengths(seed, count):
    """pairs of similar length whose shorter side runs over 1 .. 400 (one to three 160-row levels of the score sweep), the shorter
    side alpha in half of them and beta in the other half; bases incl. N"""
    rng = np.random.default_rng(seed)
    shorts = [1, 2, 159, 160, 161, 319, 320, 321, 399, 400]
    shorts += [int(x) for x in rng.integers(1, 401, size=count // 2 - len(shorts))]
    alphas, betas = [], []
    for k, s in enumerate(shorts):
        for flip in (0, 1):
            longer = s + int(rng.integers(1, s // 8 + 3))
            a = rng.integers(0, 5, size=longer).astype(np.uint8)
            b = common.mutate(rng, a, sub=0.08, indel=0.03, geo=0.4, alphabet=5)
            b = np.concatenate([b, rng.integers(0, 4, size=s).astype(np.uint8)])[:s]
            if flip:
                a, b = b, a
            alphas.append(a); betas.append(b)
    return alphas, betas


def _chunk_pairs(seed, chunk, count=24):
    """AffineGapChunk inputs: lengths of 1 .. 200 chunk cells, alpha the longer side in half of the pairs, bases incl. N"""
    rng = np.random.default_rng(seed)
    alphas, betas = [], []
    for k in range(count):
        n, m = int(rng.integers(1, 120)), int(rng.integers(121, 200))
        if k == 0:
            n, m = 161, 170  # two levels of the sweep on the shorter side
        a = rng.integers(0, 5, size=m * chunk).astype(np.uint8)
        b = common.mutate(rng, a, sub=0.1, indel=0.04, geo=0.4, alphabet=5)
        b = np.concatenate([b, rng.integers(0, 5, size=n * chunk).astype(np.uint8)])[:n * chunk]
        if k % 2:
            a, b = b, a
        alphas.append(a); betas.append(b)
    return alphas, betas


def _groups(seed, chunk, count=5):
    """alignment blocks of 1 .. 4 members with lower case and gaps, related to one root so that columns mostly agree"""
    from gonomics_amd import dna
    rng = np.random.default_rng(seed)
    groups = []
    for g in range(count):
        nseq, cells = 1 + g % 4, int(rng.integers(20, 160))
        root = rng.integers(0, 4, size=cells * chunk)
        blk = np.stack([root] * nseq).astype(np.uint8)
        sub = rng.random(blk.shape) < 0.15
        blk[sub] = rng.integers(0, 4, size=int(sub.sum()))
        low = rng.random(blk.shape) < 0.3
        blk[low] += 5  # lower case
        blk[rng.random(blk.shape) < 0.1] = dna.Gap
        blk[0, blk[0] == dna.Gap] = 1  # one member without gaps: no column pair is gap-only
        groups.append(blk)
    return groups


def _local_ref_batch(seed, count=60, ref_len=4000):
    """AffineGapLocal inputs on ONE reference (so that it can be the resident, packed one): (ref, target starts, target lengths,
    queries).  Queries of 1 .. 192 bases (one stage-2 strip of the span kernel) and of 193 .. 400 (row hand-over in device memory),
    targets shorter than their query among them, reads at both target ends and in the middle, N in the reference"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=ref_len, dtype=np.uint8)
    ref[rng.integers(0, ref_len, size=10)] = 4
    ref[2000:2040] = 4  # an N block: windows that touch it read the exception list of the packed reference
    qlens = [1, 2, 160, 161, 192, 193, 320, 321, 400] + [int(x) for x in rng.integers(3, 193, size=(count - 9) // 2)]
    qlens += [int(x) for x in rng.integers(193, 401, size=count - len(qlens))]
    t_start, t_len, queries = [], [], []
    for k, q in enumerate(qlens):
        m = [max(1, q // 3), q + 57, 700, 1500][k % 4]
        off = int(rng.integers(0, ref_len - m + 1))
        if k % 9 == 0 and m >= 700:
            off = 1700  # over the N block
        win = ref[off:off + m]
        where = (k // 4) % 3
        pos = 0 if where == 0 else (max(0, m - q) if where == 1 else int(rng.integers(0, max(1, m - q + 1))))
        if m >= q:
            read = common.mutate(rng, win[pos:pos + q + 20], 0.06, 0.02, alphabet=5)[:q]
        else:
            read = rng.integers(0, 5, size=q, dtype=np.uint8)
        if read.shape[0] < q:
            read = np.concatenate([read, rng.integers(0, 4, size=q - read.shape[0], dtype=np.uint8)])
        t_start.append(off); t_len.append(m); queries.append(np.ascontiguousarray(read, dtype=np.uint8))
    return ref, np.asarray(t_start, np.int64), np.asarray(t_len, np.int64), queries


def _global_ref_batch(seed, count=56, ref_len=4000):
    """the score sweep's batch against ONE reference: (ref, reads, window starts, window lengths), read and window of similar
    length, either one the shorter side, the shorter side 1 .. 400"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=ref_len, dtype=np.uint8)
    ref[rng.integers(0, ref_len, size=10)] = 4
    ref[2000:2040] = 4
    reads, w_start, w_len = [], [], []
    for k in range(count):
        s = [1, 160, 161, 320, 321, 400][k] if k < 6 else int(rng.integers(1, 401))
        longer = s + int(rng.integers(1, s // 8 + 3))
        n, m = (s, longer) if k % 2 else (longer, s)
        off = 1990 if k % 9 == 0 else int(rng.integers(0, ref_len - m + 1))
        read = common.mutate(rng, ref[off:off + n + 20], 0.08, 0.02, alphabet=5)[:n]
        if read.shape[0] < n:
            read = np.concatenate([read, rng.integers(0, 4, size=n - read.shape[0], dtype=np.uint8)])
        reads.append(np.ascontiguousarray(read, dtype=np.uint8)); w_start.append(off); w_len.append(m)
    return ref, reads, np.asarray(w_start, np.int64), np.asarray(w_len, np.int64)


@functools.lru_cache(maxsize=None)
def batch(name):
    """(alphas, betas) of a named batch -- for AffineGapLocal's own batches (xp*, local*) alpha is the target.  Shared: do not change them."""
    if name == "small":      # one strip, 64 pairs
        return _ragged(7001, 64, 60, 400)
    if name == "long16":     # several 160-row strips
        return _ragged(7002, 16, 700, 1500)
    if name == "long40":     # the snapshot suites' shape
        return _ragged(7003, 40, 700, 1500)
    if name == "tall12":     # tall: many strips, few columns
        return _ragged(7004, 12, 1300, 200)
    if name == "w64":        # up to 2000 x 1500, two or more 640-row strips in at least a third of the pairs
        al, be = _ragged(7005, 8, 2000, 1500)
        _, ra, rb = _related(7008, ((1300, 100, 0.05, 0.03), (1500, 0, 0.08, 0.03), (1999, 0, 0.05, 0.02), (1700, 0, 0.05, 0.03)))
        return al + ra, be + [b[:1500] for b in rb]
    if name == "coop":       # beta >= 1024: pipelined strips, wave-cooperative traceback
        al, be = common.random_pairs(7006, 8, 1, 900, 1024, 1500, related=0.8)
        al[3] = al[3][:100]
        return al, be
    if name == "panels":     # row panels: 6 related pairs of 1500 .. 3300 rows and a read inside a window
        rng, al, be = _related(7007, ((2100, 0, 0.05, 0.03), (1500, 900, 0.05, 0.03), (1700, 1500, 0.08, 0.05), (3300, 40, 0.02, 0.004),
                                      (2700, 0, 0.1, 0.02), (1900, 300, 0.05, 0.02)))
        w = rng.integers(0, 4, size=3000).astype(np.uint8)
        al.append(common.mutate(rng, w[1200:2300], sub=0.04, indel=0.03, geo=0.5)); be.append(w)
        return al, be
    if name in ("fp1", "fp2", "fp3"):
        k = int(name[2])
        return _reads_in_windows(7010 + k, 24 if k == 3 else 56, 160 * (k - 1) + 1, 160 * k)
    if name in ("xp1", "xp2", "xp3"):  # target = window, query = read
        k = int(name[2])
        reads, wins = _reads_in_windows(7020 + k, 24 if k == 3 else 56, 160 * (k - 1) + 1, 160 * k)
        return wins, reads
    if name == "fp_cheap":
        return _cheap_gap_reads(7031)
    if name == "xp_cheap":
        reads, wins = _cheap_gap_reads(7032)
        return wins, reads
    if name == "sweep":
        return _similar_lengths(7040, 56)
    if name == "local":
        ref, t_start, t_len, queries = local_ref_batch()
        return [ref[s:s + l] for s, l in zip(t_start, t_len)], queries
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def local_ref_batch():
    return _local_ref_batch(7050)


@functools.lru_cache(maxsize=None)
def global_ref_batch():
    return _global_ref_batch(7060)


@functools.lru_cache(maxsize=None)
def chunk_pairs(chunk):
    return _chunk_pairs(7070 + chunk, chunk)


@functools.lru_cache(maxsize=None)
def groups(chunk):
    """(blocks, every ordered pair of them): each pair runs as (x, y) and as (y, x)"""
    g = _groups(7080 + chunk, chunk)
    return g, [(x, y) for x in range(len(g)) for y in range(len(g)) if x != y]


@functools.lru_cache(maxsize=None)
def gsw_pairs(side):
    """200 (target, read) pairs of up to 150 x 150 -- (n + m + 2) * 600 < 2^19 -- shaped like a seed extension: the target is the read
    with 10 % substitutions and a few indels, anchored where the DP is (LeftDynamicAln ends at (n, m), RightDynamicAln starts at
    (0, 0)) and flanked on the far side; one pair in eight unrelated, N among the bases"""
    rng = np.random.default_rng(7090 + side)
    pairs = []
    for k in range(200):
        m = int(rng.integers(1, 151))
        read = rng.integers(0, 5 if k % 5 == 0 else 4, size=m).astype(np.uint8)
        if k % 8 == 7:
            target = rng.integers(0, 4, size=int(rng.integers(1, 151))).astype(np.uint8)
        else:
            core = common.mutate(rng, read, 0.1, 0.03)
            flank = rng.integers(0, 4, size=int(rng.integers(0, 12))).astype(np.uint8)
            target = (np.concatenate([core, flank])[:150] if side == 1 else np.concatenate([flank, core])[-150:]).astype(np.uint8)
        pairs.append((target, read))
    assert all(len(a) <= 150 and len(b) <= 150 and (len(a) + len(b) + 2) * 600 < (1 << 19) for a, b in pairs)
    return pairs


@functools.lru_cache(maxsize=None)
def best_of_workload():
    """about 40 reads of 30 .. 200 bases, 2 .. 4 candidate windows each, both strands (tests/test_best_of_gpu.py's generator)"""
    from test_best_of_gpu import _workload
    return _workload(7100, 40, kmax=4, kmin=2, short=(30, 100), long=(100, 200), target_len=6000)


@functools.lru_cache(maxsize=None)
def expected(name, mode, mname, go, ge, ci=10000):
    """the oracle's (scores, ops, offsets) of a named batch: computed once, shared by every route that must reproduce it"""
    alphas, betas = batch(name)
    return oracle.align_batch(mode, MATRICES[mname], go, ge, alphas, betas, ci, ci, threads=8)


@functools.lru_cache(maxsize=None)
def tells(name, mode, go, ge, other="ASYM_T", ci=10000):
    """assert_tells_orientation on a named batch, once per (batch, mode, penalties)"""
    alphas, betas = batch(name)
    assert_tells_orientation(mode, go, ge, alphas, betas, other=MATRICES[other], ci=ci, cj=ci)
    return True


# (batch, modes) of every align-route test of tests/test_asym_gpu.py: what the CPU suite checks the condition on
ALIGN_BATCHES = [("small", (0, 1, 2, 3, 4)), ("long16", (0, 1, 2, 3, 4)), ("coop", (0, 1, 2, 3, 4)), ("tall12", (0, 1, 2, 3, 4)),
                 ("long40", (0, 1, 2, 4)), ("w64", (0, 1, 2, 4)), ("panels", (0, 1, 2, 4)),
                 ("fp1", (0,)), ("fp2", (0,)), ("fp3", (0,)), ("xp1", (3,)), ("xp2", (3,)), ("xp3", (3,)),
                 ("sweep", (0, 1, 2, 4)), ("local", (3,))]
