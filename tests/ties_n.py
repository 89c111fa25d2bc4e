"""Helpers of the tie-breaking tests of the chunk / group DPs (N1) and the graph aligner's seed-extension DPs (N2):
tests/test_ties_n_cpu.py, tests/test_ties_n_gpu.py; DESIGN.md 4.33.  The sequel of tests/ties.py, whose orders, tables, sets,
sources and affine walk it uses.

  * N1 (oracle/gnx_oracle.c or_scored_affine): AffineGap_highMem's fill and walk over an explicit per-pair score matrix -- the sum of
    table entries over a chunk, or the truncated column averages of two groups; gapExtend times the chunk, gapOpen not; sites M, I, D
    and `final`, no checkerboard.  fill_scored() restates the fill row by row on numpy (the I row is a running maximum), keeps per cell
    which candidates of each argmax are maximal, and ties._walk walks the codes under an order of preference;
  * N2 (or_gsw_extend): one matrix, argmax (diagonal, left, up), site V.  Left: zero borders, cells clamped at 0, the walk from (n, m)
    while the value is positive.  Right: borders i * gap / j * gap, the first maximum in row-major order, the walk down to (0, 0).
  * decisive_n1() / decisive_ext() are the conditions that keep a batch from passing vacuously, decided by the census alone.
"""
import collections
import functools

import numpy as np

import common
import envelope
import oracle
import ties
from ties import DIM, HC2, IMD, MDI, MID, ORDERS, SET_NAME, TIE

GAP, LOWER = envelope.GAP, envelope.LOWER
VN = -(1 << 40)  # "minus infinity" in int64


def scaled(table, k):
    return [[v * k for v in row] for row in table]


# ---- the sets -----------------------------------------------------------------------------------------------------------------------
# name -> (table, gapOpen, gapExtend).  ties.AFFINE_SETS, and:
#   tie5, tie3: the tie table with gapExtend -5 / -3.  A cell of c bases with k mismatches scores 10 c - 40 k under the tie table;
#     two gaps of a chunk cost 2 e c.  Under tie15 the two are equal only at k = c (every base of the chunk a mismatch), which
#     related sequences reach often at chunk 1 alone.  10 c - 40 k = 2 e c gives e = -5 at c = 2, k = 1 (a half-mismatched chunk
#     EQUALS two gaps) and e = -3 at c = 5, k = 2; c = 3 has an integer e only at k = 3, which is tie15.  At the other chunk sizes
#     tie5 and tie3 equal no cell score: they are not run there;
#   hc3010x40: hc3010 times 40 -- the same ties cell for cell, but 4 * chunk * max|s| + |8 e chunk| leaves int16 (rule N1): the
#     score matrix is built and read as int32.
DEFAULT = common.matrices()["Default"]
N1_SETS = collections.OrderedDict(list(ties.AFFINE_SETS.items()) + [("tie5", (TIE, 0, -5)), ("tie3", (TIE, 0, -3)), ("hc3010x40", (scaled(HC2, 40), -30 * 40, -10 * 40))])
EQUAL_N1 = ("tie15", "tie5", "tie3")  # two gaps equal a cell score that occurs; in the other sets they beat a mismatch
EQUAL_AT = {"tie15": (1, 3), "tie5": (2,), "tie3": (5,)}  # ... at these chunk sizes (tie15 at 3: the all-mismatch cell)
# what tests/test_n1_gpu.py runs: (-600, -150) on the chunk batches, the default table with (-400, -30) on the groups
CONTROL_N1 = collections.OrderedDict([("c600", (HC2, -600, -150)), ("c400", (DEFAULT, -400, -30))])
CONTROL_OF = {"c_small": ("c600",), "c_long": ("c600",), "g_small": ("c600", "c400")}
EXT_SETS = collections.OrderedDict([("hc40", (HC2, -40)), ("hc70", (HC2, -70)), ("tie15", (TIE, -15))])
CONTROL_EXT = {"c600": (HC2, -600)}  # what tests/test_n2_gsw.py runs above 60 x 60


def n1_params(sname):
    return N1_SETS[sname] if sname in N1_SETS else CONTROL_N1[sname]


def ext_params(sname):
    return EXT_SETS[sname] if sname in EXT_SETS else CONTROL_EXT[sname]


def wrong_order(sname):
    """the order of preference that a batch must notice: (M, D, I) where two gaps beat a mismatch; where they equal one, M is in
    nearly every tie of I with D, and the order that demotes M is the decisive one"""
    return IMD if sname in EQUAL_N1 else MDI


# ---- the score matrices, as the reference builds them --------------------------------------------------------------------------------
def chunk_matrix(table, chunk, alpha, beta):
    """ungappedRegionScore of every pair of chunks: [n / chunk, m / chunk] int64"""
    t = np.asarray(table, np.int64)
    a, b = np.asarray(alpha, np.int64), np.asarray(beta, np.int64)
    assert len(a) % chunk == 0 and len(b) % chunk == 0
    s = np.zeros((len(a) // chunk, len(b) // chunk), np.int64)
    for k in range(chunk):
        s += t[a[k::chunk]][:, b[k::chunk]]
    return s


def _profile(block):
    """[columns, 5]: how many members of an alignment block hold base x in a column, lower case folded, gaps left out"""
    blk = np.asarray(block, np.int64)
    blk = np.where((blk >= LOWER) & (blk < GAP), blk - LOWER, blk)
    return np.stack([(blk == x).sum(axis=0) for x in range(5)], axis=1)


def group_matrix(table, chunk, block_a, block_b):
    """scoreColumnMatch / ungappedRegionColumnScore: per column pair the average over the non-gap pairs of members, truncated toward
    zero, summed over the columns of a chunk"""
    t = np.asarray(table, np.int64)
    pa, pb = _profile(block_a), _profile(block_b)
    assert len(pa) % chunk == 0 and len(pb) % chunk == 0
    s = np.zeros((len(pa) // chunk, len(pb) // chunk), np.int64)
    for k in range(chunk):
        qa, qb = pa[k::chunk], pb[k::chunk]
        total = qa @ t @ qb.T
        count = np.outer(qa.sum(axis=1), qb.sum(axis=1))
        assert count.min() > 0  # (the reference panics on a column pair of gaps alone)
        s += np.sign(total) * (np.abs(total) // count)
    return s


# ---- N1: fill and walk -----------------------------------------------------------------------------------------------------------------
def _masks(c0, c1, c2):
    mx = np.maximum(np.maximum(c0, c1), c2)
    return ((c0 == mx).astype(np.uint16) | ((c1 == mx).astype(np.uint16) << 1) | ((c2 == mx).astype(np.uint16) << 2))


def fill_scored(smat, go, ge):
    """(codes [n + 1, m + 1] in the layout of ties._fill_chunk's affine codes, final score) of or_scored_affine's fill; ge is the
    gapExtend the DP sees (times the chunk).  Row by row: M and D come from the row above, I[j] = max(Y[j-1] + e, I[j-1] + e) with
    Y = max(M, D) + gapOpen is a running maximum of Y[k] - k e."""
    n, m = smat.shape
    o, e = int(go), int(ge)
    M = np.full((n + 1, m + 1), VN, np.int64)
    I = np.full((n + 1, m + 1), VN, np.int64)
    D = np.full((n + 1, m + 1), VN, np.int64)
    cols = np.arange(m + 1, dtype=np.int64)
    M[0, 0], I[0, 0], D[0, 0] = 0, o, o
    I[0, 1:] = o + e * cols[1:]
    D[1:, 0] = o + e * np.arange(1, n + 1)
    for i in range(1, n + 1):
        M[i, 1:] = smat[i - 1] + np.maximum(np.maximum(M[i - 1, :-1], I[i - 1, :-1]), D[i - 1, :-1])
        D[i, 1:] = np.maximum(np.maximum(M[i - 1, 1:], I[i - 1, 1:]) + (o + e), D[i - 1, 1:] + e)
        y = np.maximum(M[i], D[i]) + o - e * cols  # y[k] + e * j = Y[k] + (j - k) e
        I[i, 1:] = np.maximum.accumulate(y)[:-1] + e * cols[1:]  # (I[i][0] is "minus infinity": it never wins)
    oe = o + e
    code = np.zeros((n + 1, m + 1), np.uint16)
    code[1:, 1:] = (_masks(M[:-1, :-1], I[:-1, :-1], D[:-1, :-1]) | (_masks(M[1:, :-1] + oe, I[1:, :-1] + e, D[1:, :-1] + oe) << 3)
                    | (_masks(M[:-1, 1:] + oe, I[:-1, 1:] + oe, D[:-1, 1:] + e) << 6) | (_masks(M[1:, 1:], I[1:, 1:], D[1:, 1:]) << 9))
    return code, int(max(M[n, m], I[n, m], D[n, m]))


BIG = 1 << 60  # a checkerboard no pair reaches: ties._walk is then AffineGap_highMem's walk, which is or_scored_affine's


def walk_scored(smat, go, ge, chunk, orders=(MID,)):
    """{order: (score, route [(run, op)] with the runs times the chunk, ties [(site, tied set, i, j)])}"""
    n, m = smat.shape
    assert n > 0 and m > 0
    code, score = fill_scored(smat, go, ge * chunk)
    out = {}
    for o in orders:
        route, tied = ties._walk("affine", code, n, m, BIG, BIG, o)
        out[o] = (score, [(r * chunk, op) for r, op in route], tied)
    return out


# ---- N2: fill and walk -----------------------------------------------------------------------------------------------------------------
def fill_ext(side, table, gap, alpha, beta):
    """(V [n + 1, m + 1] int64, codes [n + 1, m + 1]: bits 0-2 the maximal candidates (diagonal, left, up) of a cell) of
    LeftDynamicAln (side 0) / RightDynamicAln (side 1).  V[i][j] = max(X[j], V[i][j-1] + gap), X from the row above (and the clamp
    at 0 on the left side): a running maximum of X[k] - k gap."""
    n, m = len(alpha), len(beta)
    g = int(gap)
    s = np.asarray(table, np.int64)[np.asarray(alpha, np.int64)][:, np.asarray(beta, np.int64)]
    V = np.zeros((n + 1, m + 1), np.int64)
    cols = np.arange(m + 1, dtype=np.int64)
    if side == 1:
        V[0] = g * cols
    x = np.zeros(m + 1, np.int64)
    for i in range(1, n + 1):
        x[0] = g * i if side == 1 else 0
        x[1:] = np.maximum(V[i - 1, :-1] + s[i - 1], V[i - 1, 1:] + g)
        if side == 0:
            np.maximum(x, 0, out=x)
        V[i] = np.maximum.accumulate(x - g * cols) + g * cols
    code = np.zeros((n + 1, m + 1), np.uint16)
    code[1:, 1:] = _masks(V[:-1, :-1] + s, V[1:, :-1] + g, V[:-1, 1:] + g)
    return V, code


def _rle(ops):
    out = []
    for op in ops:
        if out and out[-1][1] == op:
            out[-1][0] += 1
        else:
            out.append([1, op])
    return [(r, o) for r, o in out]


def walk_ext(side, V, code, order):
    """(score, route in traceback order, end i, end j, ties [("V", tied set, i, j)]) as or_gsw_extend returns them"""
    ch = ties._chooser(order)
    n, m = V.shape[0] - 1, V.shape[1] - 1
    ops, tied = [], []
    if side == 0:
        i, j = n, m
        score = int(V[n, m])
        while V[i, j] > 0:
            mk = int(code[i, j])
            k = ch[mk]
            if mk in SET_NAME:
                tied.append(("V", SET_NAME[mk], i, j))
            ops.append(k)
            i, j = i - (k != 1), j - (k != 2)
        return score, _rle(ops), i, j, tied
    best = int(V.max())
    bi, bj = (0, 0) if best <= 0 else (int(x) for x in np.unravel_index(int(np.argmax(V)), V.shape))  # (argmax: the first in row-major order)
    i, j = bi, bj
    while i > 0 or j > 0:
        if i == 0:
            k = 1
        elif j == 0:
            k = 2
        else:
            mk = int(code[i, j])
            k = ch[mk]
            if mk in SET_NAME:
                tied.append(("V", SET_NAME[mk], i, j))
        ops.append(k)
        i, j = i - (k != 1), j - (k != 2)
    return int(V[bi, bj]), _rle(ops), bi, bj, tied


def max_cells(V):
    """the cells that hold RightDynamicAln's maximum (none when nothing is positive: the walk then starts at (0, 0))"""
    best = int(V.max())
    return [] if best <= 0 else [(int(i), int(j)) for i, j in np.argwhere(V == best)]


# ---- the batches ----------------------------------------------------------------------------------------------------------------------
def _mutate_cells(rng, x, chunk, sub, indel, geo=0.5):
    """a copy of x (whole chunks): substitutions per base, indels of whole chunks (geometric lengths, in chunks)"""
    cells = np.asarray(x, np.uint8).reshape(-1, chunk)
    out, i = [], 0
    while i < len(cells):
        r = rng.random()
        if r < indel / 2:
            i += int(rng.geometric(geo))
            continue
        if r < indel:
            out.extend(rng.integers(0, 4, size=(int(rng.geometric(geo)), chunk)).astype(np.uint8))
        out.append(cells[i])
        i += 1
    y = np.asarray(out if out else [cells[0]], np.uint8).reshape(-1)
    hit = rng.random(len(y)) < sub
    y[hit] = rng.integers(0, 4, size=int(hit.sum()))
    return y


def _chunk_pair(rng, k, n, m, chunk, sub, indel):
    """ties._pair in chunk cells: pair k is of kind k % 3 (four letters, two letters, tandem repeat), one side a copy of the other
    with substitutions per base and indels of whole chunks (three times as many in the repeat kinds), the shorter side cut from
    inside the longer one's span, the sides exchanged in every other pair of a kind"""
    kind, flip = k % 3, (k // 3) % 2
    length = (max(n, m) + 24) * chunk
    x = ties._source(rng, kind, length)
    y = _mutate_cells(rng, x, chunk, sub, indel * (1 if kind == 0 else 3))
    if len(y) < length:
        y = np.concatenate([y, ties._source(rng, kind, length - len(y))])
    sa, sb = (y, x) if flip else (x, y)
    if n <= m:
        off = int(rng.integers(0, m - n + 1)) * chunk
        a, b = sa[off:off + n * chunk], sb[:m * chunk]
    else:
        off = int(rng.integers(0, n - m + 1)) * chunk
        a, b = sa[:n * chunk], sb[off:off + m * chunk]
    return np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)


C_SHAPES = {  # lengths in chunk cells
    "c_small": lambda: ties._shapes(9101, 24, 40, 150, 40, 190, fixed=((160, 160), (1, 30), (30, 1))),
    "c_long": lambda: ties._shapes(9102, 10, 170, 450, 200, 600, fixed=((321, 330), (257, 300), (450, 600), (170, 512))),
}
C_CHUNKS = {"c_small": (1, 2, 3, 5), "c_long": (1, 3)}
G_CHUNKS = (1, 2)


@functools.lru_cache(maxsize=None)
def chunk_batch(name, chunk):
    """(alphas, betas) of a named N1 batch at a chunk size.  Shared: do not change them."""
    rng = np.random.default_rng({"c_small": 9001, "c_long": 9002}[name] + 10 * chunk)
    pairs = [_chunk_pair(rng, k, n, m, chunk, 0.05, 0.08) for k, (n, m) in enumerate(C_SHAPES[name]())]
    return [a for a, _ in pairs], [b for _, b in pairs]


@functools.lru_cache(maxsize=None)
def group_batch(chunk):
    """(blocks, every ordered pair of them): 8 alignment blocks of 1 .. 4 members over 40 .. 200 chunk cells.  One source in three
    stretches (four letters, two letters, a tandem repeat); a block is a window of a mutated copy of it (indels of whole chunks),
    its members copies of that with a few substitutions, lower case in a third of the bases and 10 % gaps except in the first row
    (no column pair is gap-only): the second block of every pair is a mutated copy of the first one's source"""
    rng = np.random.default_rng(9003 + 10 * chunk)
    cells = 224
    source = np.concatenate([ties._source(rng, kind, 75 * chunk) for kind in (0, 1, 2)])[:cells * chunk]
    lengths = [200, 40] + [int(x) for x in rng.integers(60, 201, size=6)]
    members = [1, 4, 2, 3, 1, 2, 3, 4]
    blocks = []
    for g, (ln, nseq) in enumerate(zip(lengths, members)):
        y = _mutate_cells(rng, source, chunk, 0.03, 0.08)
        y = np.concatenate([y, ties._source(rng, 0, cells * chunk)])[:cells * chunk]
        off = int(rng.integers(0, cells - ln + 1)) * chunk
        row = y[off:off + ln * chunk]
        blk = np.stack([row] * nseq).astype(np.uint8)
        hit = rng.random(blk.shape) < 0.04
        hit[0] = False
        blk[hit] = rng.integers(0, 4, size=int(hit.sum()))
        blk[rng.random(blk.shape) < 0.3] += LOWER
        gaps = rng.random(blk.shape) < 0.1
        gaps[0] = False
        blk[gaps] = GAP
        blocks.append(np.ascontiguousarray(blk))
    return blocks, [(x, y) for x in range(len(blocks)) for y in range(len(blocks)) if x != y]


def _ext_pair(rng, k, n, m, side):
    """(target of n rows, read of m columns) anchored as tests/test_n2_gsw.py anchors them: the read is a copy with errors of the
    target's anchored end -- its first bases for RightDynamicAln, which starts at (0, 0), its last ones for LeftDynamicAln, which ends
    at (n, m).  Kinds as ties._pair; in every fourth pair the third of the read farthest from the anchor is unrelated to the target
    (the extension then ends inside the matrix where the penalties let a score die out)"""
    kind = k % 3
    alpha = ties._source(rng, kind, n)
    part = alpha[:m + 8] if side == 1 else alpha[max(n - m - 8, 0):]
    beta = common.mutate(rng, part, sub=0.05, indel=0.04 * (1 if kind == 0 else 3), geo=0.5)
    beta = beta[:m] if side == 1 else beta[max(len(beta) - m, 0):]
    fill = ties._source(rng, 0, m - len(beta))
    beta = np.concatenate([beta, fill] if side == 1 else [fill, beta])
    if k % 4 == 3 and m >= 6:
        junk = rng.integers(0, 4, size=m // 3).astype(np.uint8)
        beta = np.concatenate([beta[:m - len(junk)], junk] if side == 1 else [junk, beta[len(junk):]])
    assert (len(alpha), len(beta)) == (n, m)
    return np.ascontiguousarray(alpha, np.uint8), np.ascontiguousarray(beta, np.uint8)


def _piped_shapes():
    rng = np.random.default_rng(9113)
    out = [(170, 800), (600, 512), (321, 640)]
    while len(out) < 8:
        m = int(rng.integers(512, 801))
        out.append((int(rng.integers(170, min(600, 1470 - m) + 1)), m))
    return out


X_SHAPES = {
    "x_small": lambda: ties._shapes(9111, 30, 20, 160, 20, 150, fixed=((160, 150), (1, 20), (20, 1), (159, 16))),
    "x_multi": lambda: ties._shapes(9112, 12, 161, 700, 100, 400, fixed=((161, 100), (320, 400), (321, 333), (700, 250))),
    "x_piped": _piped_shapes,
}
X_SEEDS = {"x_small": 9011, "x_multi": 9012, "x_piped": 9023}
CROSS = ((100, 40), (330, 30), (300, 30))  # (p, q) of the constructed pairs: strips 0 and 1, both in strip 2, strips 1 and 2
STRIP = 160


@functools.lru_cache(maxsize=None)
def ext_batch(name, side):
    """(targets, reads) of a named extension batch for a side.  Shared: do not change them."""
    if name == "x_cross":
        return cross_pairs()
    rng = np.random.default_rng(X_SEEDS[name] + side)
    pairs = [_ext_pair(rng, k, n, m, side) for k, (n, m) in enumerate(X_SHAPES[name]())]
    return [a for a, _ in pairs], [b for _, b in pairs]


def cross_pairs():
    """RightDynamicAln keeps the FIRST maximum in row-major order.  Under the tie table and gap -15: target A x p + C x q + A x 3q,
    read A x p + G x q + A x 3q + T x r.  The score reaches 10 p at (p, p), falls by 30 a mismatch (or by 15 a gap, two of them for
    a C and a G: the same), and the 3q matches behind buy it back to exactly 10 p at (p + 4q, p + 4q), the target's last row.  The
    tail of T (no match anywhere) makes the read 520 columns or more: the piped launch."""
    al, be = [], []
    for p, q in CROSS:
        al.append(np.concatenate([np.zeros(p, np.uint8), np.full(q, 1, np.uint8), np.zeros(3 * q, np.uint8)]))
        be.append(np.concatenate([np.zeros(p, np.uint8), np.full(q, 2, np.uint8), np.zeros(3 * q, np.uint8), np.full(max(520 - p - 4 * q, 60), 3, np.uint8)]))
    return al, be


# ---- what is run: (batch, chunk) -> sets ---------------------------------------------------------------------------------------------
# Every set costs a fill of every pair on the CPU.  Each (batch, chunk) keeps sets in which two gaps beat a mismatch and one in which
# they equal a cell score (EQUAL_AT).  NOT_RUN: the sets the census shows unable to meet the conditions at a chunk size
# (tests/test_ties_n_cpu.py keeps that on record: each of them must fail decisive_n1).  From chunk 2 on a cell with ONE mismatch
# among its bases costs less than two gaps of a chunk under hc70 (90 - 330 against -280 at chunk 2), and from chunk 5 on under hc40
# too: (M, D, I) then changes fewer than half of the pairs of c_small.  At chunk 3 and on the long and group batches the indels of
# whole chunks inside repeats still tie I with D on most routes, and the sets stay.
N1_PLAN = collections.OrderedDict([
    (("c_small", 1), ("hc70", "hc3010", "hc40", "tie15")),
    (("c_small", 2), ("hc3010", "hc40", "tie5")),
    (("c_small", 3), ("hc70", "hc3010", "tie15")),
    (("c_small", 5), ("hc3010", "hc3010x40", "tie3")),
    (("c_long", 1), ("hc70", "hc3010", "tie15")),
    (("c_long", 3), ("hc70", "hc3010", "tie15")),
    (("g_small", 1), ("hc70", "hc3010", "tie15")),
    (("g_small", 2), ("hc3010", "hc3010x40", "tie5")),
])
NOT_RUN = ((("c_small", 2), "hc70"), (("c_small", 5), "hc70"), (("c_small", 5), "hc40"))
EXT_PLAN = collections.OrderedDict([("x_small", ("hc40", "hc70", "tie15")), ("x_multi", ("hc40", "hc70", "tie15")), ("x_piped", ("hc40", "hc70", "tie15"))])


def n1_matrices(name, chunk, table):
    if name == "g_small":
        blocks, pairs = group_batch(chunk)
        return [group_matrix(table, chunk, blocks[x], blocks[y]) for x, y in pairs]
    al, be = chunk_batch(name, chunk)
    return [chunk_matrix(table, chunk, a, b) for a, b in zip(al, be)]


@functools.lru_cache(maxsize=None)
def n1_runs(name, chunk, sname):
    """{order: [(score, route, ties) per pair]} of a batch under one set"""
    table, go, ge = n1_params(sname)
    orders = ORDERS if sname in N1_SETS else (MID, MDI)
    rows = [walk_scored(s, go, ge, chunk, orders) for s in n1_matrices(name, chunk, table)]
    return {o: [r[o] for r in rows] for o in orders}


@functools.lru_cache(maxsize=None)
def n1_expected(name, chunk, sname):
    """the oracle's [(score, route)]: computed once, shared by every route that must reproduce it"""
    table, go, ge = n1_params(sname)
    if name == "g_small":
        blocks, pairs = group_batch(chunk)
        return [oracle.multiple_affine_gap(table, go, ge, chunk, blocks[x], blocks[y]) for x, y in pairs]
    al, be = chunk_batch(name, chunk)
    return [oracle.affine_gap_chunk(table, go, ge, chunk, a, b) for a, b in zip(al, be)]


def n1_counts(name, chunk, sname, order=MID):
    return [collections.Counter((s, t) for s, t, _, _ in tied) for _, _, tied in n1_runs(name, chunk, sname)[order]]


def n1_changed(name, chunk, sname, order):
    runs = n1_runs(name, chunk, sname)
    return [r[1] != q[1] for r, q in zip(runs[order], runs[MID])]


@functools.lru_cache(maxsize=None)
def ext_runs(name, side, sname):
    """{order: [(score, route, i, j, ties) per pair]}, and per pair the cells that hold the maximum (right side)"""
    table, gap = ext_params(sname)
    orders = ORDERS if sname in EXT_SETS else (MID, MDI)
    out, cells = {o: [] for o in orders}, []
    for a, b in zip(*ext_batch(name, side)):
        V, code = fill_ext(side, table, gap, a, b)
        for o in orders:
            out[o].append(walk_ext(side, V, code, o))
        cells.append(max_cells(V) if side == 1 else None)
    return out, cells


@functools.lru_cache(maxsize=None)
def ext_expected(name, side, sname):
    table, gap = ext_params(sname)
    return [oracle.gsw_extend(side, table, gap, a, b) for a, b in zip(*ext_batch(name, side))]


def ext_counts(name, side, sname):
    return [collections.Counter((s, t) for s, t, _, _ in r[4]) for r in ext_runs(name, side, sname)[0][MID]]


def ext_changed(name, side, sname, order):
    runs = ext_runs(name, side, sname)[0]
    return [r[:4] != q[:4] for r, q in zip(runs[order], runs[MID])]


def left_end(name, sname):
    """per pair of a left-side batch: "none" (nothing positive at (n, m)), "border" or "clamped" (an interior cell of value 0)"""
    return ["none" if not r[1] else ("border" if r[2] == 0 or r[3] == 0 else "clamped") for r in ext_runs(name, 0, sname)[0][MID]]


# ---- the conditions ---------------------------------------------------------------------------------------------------------------
MIN_PAIRS, MIN_CELLS = ties.MIN_PAIRS, ties.MIN_CELLS
REQUIRED_N1 = list(ties.REQUIRED)          # M and I sites, D MD: the table of DESIGN.md 4.32 without Q1 (there is no checkerboard)
REQUIRED_EXT = list(ties.REQUIRED_CONST)   # V
# EXEMPT_*: the classes a batch does not reach under a set (fewer than MIN_PAIRS pairs or MIN_CELLS cells), from the census; every
# other class is required there, a stale entry fails tests/test_ties_n_cpu.py, and no batch is exempt from a class under every set
# it runs.  The reasons are those of ties.EXEMPT: where two gaps BEAT every mismatch "MID" at M and V needs both neighbours exactly a
# cell score and a gap above the diagonal one; with gapOpen < 0 (hc3010) a tie in the I or D recurrence asks M + gapOpen = I exactly;
# where two gaps EQUAL a cell score M joins every tie of I with D ("MID" takes the place of "ID"), and the I site's "MD" and "ID",
# which need a D candidate above M's, do not occur.  Sums over a chunk and column averages thin the exact equalities further.
EXEMPT_N1 = {  # (batch, chunk, set)
    ('c_small', 1, 'hc70'): (('M', 'MID'),),
    ('c_small', 1, 'hc3010'): (('M', 'MID'), ('I', 'ID')),
    ('c_small', 1, 'hc40'): (('M', 'MID'),),
    ('c_small', 1, 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('c_small', 2, 'hc3010'): (('M', 'MID'), ('I', 'MD')),
    ('c_small', 2, 'hc40'): (('M', 'MID'), ('I', 'MD')),
    ('c_small', 2, 'tie5'): (('I', 'MD'),),
    ('c_small', 3, 'hc70'): (('M', 'MID'), ('I', 'MD')),
    ('c_small', 3, 'hc3010'): (('M', 'MD'), ('M', 'MID'), ('I', 'MD'), ('D', 'MD')),
    ('c_small', 3, 'tie15'): (('M', 'ID'), ('M', 'MID'), ('I', 'MD'), ('I', 'ID')),
    ('c_small', 5, 'hc3010'): (('M', 'MD'), ('M', 'MID'), ('I', 'MI'), ('I', 'MD'), ('I', 'ID'), ('D', 'MD')),
    ('c_small', 5, 'hc3010x40'): (('M', 'MD'), ('M', 'MID'), ('I', 'MI'), ('I', 'MD'), ('I', 'ID'), ('D', 'MD')),
    ('c_small', 5, 'tie3'): (('I', 'MD'), ('D', 'MD')),
    ('c_long', 1, 'hc70'): (('M', 'MID'),),
    ('c_long', 1, 'hc3010'): (('M', 'MID'), ('D', 'MD')),
    ('c_long', 1, 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('c_long', 3, 'hc70'): (('M', 'MID'), ('I', 'MD'), ('D', 'MD')),
    ('c_long', 3, 'hc3010'): (('M', 'MID'), ('I', 'MD'), ('D', 'MD')),
    ('c_long', 3, 'tie15'): (('M', 'ID'), ('I', 'MD'), ('I', 'ID'), ('D', 'MD')),
    ('g_small', 1, 'hc70'): (('M', 'MID'),),
    ('g_small', 1, 'hc3010'): (('M', 'MID'),),
    ('g_small', 1, 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('g_small', 2, 'hc3010'): (('M', 'MID'),),
    ('g_small', 2, 'hc3010x40'): (('M', 'MID'),),
}
EXEMPT_EXT = {  # (batch, side, set)
    ('x_small', 0, 'hc40'): (('V', 'MID'),),
    ('x_small', 0, 'hc70'): (('V', 'MID'),),
    ('x_small', 0, 'tie15'): (('V', 'ID'),),
    ('x_small', 1, 'hc40'): (('V', 'MID'),),
    ('x_small', 1, 'hc70'): (('V', 'MID'),),
    ('x_small', 1, 'tie15'): (('V', 'ID'),),
    ('x_multi', 0, 'hc40'): (('V', 'MID'),),
    ('x_multi', 0, 'hc70'): (('V', 'MID'),),
    ('x_multi', 0, 'tie15'): (('V', 'ID'),),
    ('x_multi', 1, 'hc40'): (('V', 'MID'),),
    ('x_multi', 1, 'hc70'): (('V', 'MID'),),
    ('x_piped', 0, 'hc40'): (('V', 'MID'),),
    ('x_piped', 0, 'hc70'): (('V', 'MID'),),
    ('x_piped', 1, 'hc40'): (('V', 'MID'),),
    ('x_piped', 1, 'hc70'): (('V', 'MID'),),
}


def required_n1(name, chunk, sname):
    skip = EXEMPT_N1.get((name, chunk, sname), ())
    return [c for c in REQUIRED_N1 if c not in skip]


def required_ext(name, side, sname):
    skip = EXEMPT_EXT.get((name, side, sname), ())
    return [c for c in REQUIRED_EXT if c not in skip]


def _same_n1(rows, exp, what):
    for p, (r, x) in enumerate(zip(rows, exp)):
        assert (r[0], r[1]) == x, "census walk against the oracle: %s pair %d" % (what, p)


@functools.lru_cache(maxsize=None)
def decisive_n1(name, chunk, sname):
    """On the census of the reference's route alone: the census' own walk equals the oracle; the wrong order of the set changes at
    least half of the pairs; where two gaps beat a mismatch a tie with I and D both in the tied set lies on the route of at least
    half; every required class on at least MIN_PAIRS pairs and MIN_CELLS cells; a tied final state on at least one pair.  Raises."""
    what = "%s chunk %d %s" % (name, chunk, sname)
    _same_n1(n1_runs(name, chunk, sname)[MID], n1_expected(name, chunk, sname), what)
    cnts = n1_counts(name, chunk, sname)
    ch = sum(n1_changed(name, chunk, sname, wrong_order(sname)))
    assert 2 * ch >= len(cnts), "the wrong order changes only %d of %d pairs (%s)" % (ch, len(cnts), what)
    if sname not in EQUAL_N1:
        idt = sum(ties.has_id(c) for c in cnts)
        assert 2 * idt >= len(cnts), "only %d of %d pairs have an I/D tie on their route (%s)" % (idt, len(cnts), what)
    for cls in required_n1(name, chunk, sname):
        pairs, cells = sum(1 for c in cnts if c[cls]), sum(c[cls] for c in cnts)
        assert pairs >= MIN_PAIRS and cells >= MIN_CELLS, "class %s %s: %d pairs, %d cells (%s)" % (cls + (pairs, cells, what))
    assert any(c[("final", t)] for c in cnts for t in SET_NAME.values()), "no tied final state (%s)" % what
    return True


LEFT_CLAMPED_MIN = 3


@functools.lru_cache(maxsize=None)
def decisive_ext(name, side, sname):
    """The same for an extension batch, with score and end (i, j) part of the equality; on the left side, under the equal-cost set
    the walk ends at an interior clamped cell on at least LEFT_CLAMPED_MIN pairs, under the cheap-gap sets on a border on at least half."""
    what = "%s side %d %s" % (name, side, sname)
    rows, exp = ext_runs(name, side, sname)[0][MID], ext_expected(name, side, sname)
    for p, (r, x) in enumerate(zip(rows, exp)):
        assert r[:4] == x, "census walk against the oracle: %s pair %d" % (what, p)
    cnts = ext_counts(name, side, sname)
    ch = sum(ext_changed(name, side, sname, wrong_order(sname)))
    assert 2 * ch >= len(cnts), "the wrong order changes only %d of %d pairs (%s)" % (ch, len(cnts), what)
    if sname not in EQUAL_N1:
        idt = sum(ties.has_id(c) for c in cnts)
        assert 2 * idt >= len(cnts), "only %d of %d pairs have an I/D tie on their route (%s)" % (idt, len(cnts), what)
    for cls in required_ext(name, side, sname):
        pairs, cells = sum(1 for c in cnts if c[cls]), sum(c[cls] for c in cnts)
        assert pairs >= MIN_PAIRS and cells >= MIN_CELLS, "class %s %s: %d pairs, %d cells (%s)" % (cls + (pairs, cells, what))
    if side == 0:
        ends = left_end(name, sname)
        if sname in EQUAL_N1:
            assert ends.count("clamped") >= LEFT_CLAMPED_MIN, (what, collections.Counter(ends))
        else:
            assert 2 * ends.count("border") >= len(ends), (what, collections.Counter(ends))
    return True


@functools.lru_cache(maxsize=None)
def cross_condition():
    """the constructed pairs: the maximum 10 p in exactly two cells, (p, p) and (p + 4q, p + 4q), in the strips CROSS names; the
    census walk equals the oracle, which ends at the first.  Returns the ends."""
    table, gap = EXT_SETS["tie15"]
    al, be = cross_pairs()
    strips = []
    for (p, q), a, b in zip(CROSS, al, be):
        assert len(b) >= 512
        V, code = fill_ext(1, table, gap, a, b)
        assert max_cells(V) == [(p, p), (p + 4 * q, p + 4 * q)] and int(V[p, p]) == 10 * p, (p, q, max_cells(V)[:4])
        assert walk_ext(1, V, code, MID)[:4] == oracle.gsw_extend(1, table, gap, a, b) and oracle.gsw_extend(1, table, gap, a, b)[2:] == (p, p)
        V0, code0 = fill_ext(0, table, gap, a, b)
        assert walk_ext(0, V0, code0, MID)[:4] == oracle.gsw_extend(0, table, gap, a, b)
        strips.append(((p - 1) // STRIP, (p + 4 * q - 1) // STRIP))
    assert strips == [(0, 1), (2, 2), (1, 2)], strips
    return tuple((p, p) for p, _ in CROSS)


def table_row(cnts):
    """{class: (pairs, cells)} of a census, for DESIGN.md's tables"""
    keys = sorted({k for c in cnts for k in c})
    return collections.OrderedDict((k, (sum(1 for c in cnts if c[k]), sum(c[k] for c in cnts))) for k in keys)
