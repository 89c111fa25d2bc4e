"""Helpers of the tie-breaking tests (tests/test_ties_cpu.py, tests/test_ties_gpu.py).

Every CIGAR is promised bit-exact, so every kernel family has to break ties as the reference's tripleMaxTrace does -- M over I over D --
in the three recurrences, in the final state, in the restart after an upward exit of a checkerboard (quirk Q1) and in the constant-gap
argmax.  Under the penalty sets the other suites use a mismatch costs less than two gaps, I and D never tie above M on an optimal
path, and a kernel that prefers D over I passes them all.  Here:

  * census() restates the walk of tests/pyref.py on numpy matrices filled along anti-diagonals and counts, per pair, the tied argmaxes
    the walk CONSULTS, by class (site, tied set).  At such a cell another order of preference takes another branch, so the CIGAR
    differs: the census is a statement about decisiveness.  The same walk takes an `order`; under (M, I, D) it is the oracle's;
  * the penalty sets make two gaps beat every mismatch (or equal it: TIE), the batches have the shapes of tests/asym.py's routes;
  * decisive() is the condition that keeps a batch from passing vacuously, decided on the CPU by the census alone.
"""
import collections
import functools

import numpy as np

import common
import oracle

MID, MDI, IMD, DIM = (0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 1, 0)  # orders of preference; MID is tripleMaxTrace's
ORDERS = (MID, MDI, IMD, DIM)
SET_NAME = {3: "MI", 5: "MD", 6: "ID", 7: "MID"}  # bit 0: M, bit 1: I, bit 2: D are among the maxima
SITE_NAME = ("M", "I", "D")
AFFINE_MODES = (0, 2, 3)
LOWMEM = (0, 1)

HC2 = [[90, -330, -236, -356, -208], [-330, 100, -318, -236, -196], [-236, -318, 100, -330, -196], [-356, -236, -330, 90, -208],
       [-208, -196, -196, -208, -202]]  # align.HumanChimpTwoScoreMatrix (tests/test_ties_cpu.py checks it is)
TIE = [[10 if a == b else -30 for b in range(4)] + [-10] for a in range(4)] + [[-10] * 5]  # a mismatch EQUALS two gaps of -15

# name -> (table, gapOpen, gapExtend); the constant-gap sets have gapExtend 0
AFFINE_SETS = collections.OrderedDict([("hc70", (HC2, 0, -70)), ("hc3010", (HC2, -30, -10)), ("hc40", (HC2, 0, -40)), ("tie15", (TIE, 0, -15))])
CONST_SETS = collections.OrderedDict([("hc40", (HC2, -40, 0)), ("hc70", (HC2, -70, 0)), ("tie15", (TIE, -15, 0))])
CONTROL = {"affine": (HC2, -600, -150), "const": (HC2, -430, 0)}  # what the route suites use: blind to I against D


def kind_of(mode):
    return "local" if mode == 3 else ("affine" if mode in AFFINE_MODES else "const")


def sets(mode):
    return AFFINE_SETS if mode in AFFINE_MODES else CONST_SETS


def params(mode, sname):
    if sname == "control":
        return CONTROL["affine" if mode in AFFINE_MODES else "const"]
    return sets(mode)[sname]


# ---- the fill: per cell, which of the candidates of each argmax are maximal -------------------------------------------------------------
VN = -(1 << 29)  # "minus infinity" in int32: below every score of these sizes, far from overflow
CELL_LIMIT = 20 << 20  # cells of one chunk of pairs filled together


def _masks(c0, c1, c2):
    mx = np.maximum(np.maximum(c0, c1), c2)
    return mx, (c0 == mx).view(np.uint8) | ((c1 == mx).view(np.uint8) << 1) | ((c2 == mx).view(np.uint8) << 2)


def _fill_chunk(kind, table, go, ge, al, be):
    """codes [P, N + 1, M + 1] (uint16) and final scores of P pairs, padded to the largest.  Affine: bits 0-2 / 3-5 / 6-8 the maximal
    candidates (from M, from I, from D) of the M / I / D recurrence of the cell, bits 9-11 the maxima among M, I, D of the cell itself
    (final state, Q1).  Constant gap: bits 0-2 the maximal candidates (diagonal, left, up) of V."""
    P = len(al)
    ns, ms = np.array([len(a) for a in al]), np.array([len(b) for b in be])
    N, Mx = int(ns.max()), int(ms.max())
    a5 = np.zeros((P, N), np.int64)
    bb = np.zeros((P, Mx), np.int64)
    for p in range(P):
        a5[p, :ns[p]] = np.asarray(al[p], np.int64) * 5
        bb[p, :ms[p]] = be[p]
    tf = np.asarray(table, np.int32).ravel()
    code = np.zeros((P, N + 1, Mx + 1), np.uint16)
    score = np.zeros(P, np.int64)
    end_d = ns + ms
    affine = kind != "const"
    free_end = kind == "local"
    oe, e = np.int32(go + ge), np.int32(ge)
    g = np.int32(go)
    nb = 3 if affine else 1
    bufs = [[np.full((P, N + 1), VN, np.int32) for _ in range(nb)] for _ in range(3)]
    cur = bufs[0]
    if affine:
        cur[0][:, 0], cur[1][:, 0], cur[2][:, 0] = 0, go, (0 if free_end else go)
    else:
        cur[0][:, 0] = 0
    prev2, prev1 = None, cur
    for d in range(1, N + Mx + 1):
        cur = bufs[d % 3]
        a, b = max(1, d - Mx), min(d - 1, N)
        if a <= b:
            ia, ic = slice(a - 1, b), slice(a, b + 1)
            iarr = np.arange(a, b + 1)
            s = tf[a5[:, a - 1:b] + bb[:, d - b - 1:d - a][:, ::-1]]
            if affine:
                mx, cm = _masks(prev2[0][:, ia], prev2[1][:, ia], prev2[2][:, ia])
                cur[0][:, ic] = s + mx
                mx, ci_ = _masks(prev1[0][:, ic] + oe, prev1[1][:, ic] + e, prev1[2][:, ic] + oe)
                cur[1][:, ic] = mx
                if free_end:  # (AffineGapLocal: the target's rows past the query's end cost nothing)
                    fe = (d - iarr)[None, :] == ms[:, None]
                    od, ed = np.where(fe, np.int32(0), oe), np.where(fe, np.int32(0), e)
                else:
                    od, ed = oe, e
                mx, cd = _masks(prev1[0][:, ia] + od, prev1[1][:, ia] + od, prev1[2][:, ia] + ed)
                cur[2][:, ic] = mx
                _, cc = _masks(cur[0][:, ic], cur[1][:, ic], cur[2][:, ic])
                code[:, iarr, d - iarr] = cm.astype(np.uint16) | (ci_.astype(np.uint16) << 3) | (cd.astype(np.uint16) << 6) | (cc.astype(np.uint16) << 9)
            else:
                mx, cv = _masks(prev2[0][:, ia] + s, prev1[0][:, ic] + g, prev1[0][:, ia] + g)
                cur[0][:, ic] = mx
                code[:, iarr, d - iarr] = cv
        if d <= Mx:  # row 0
            if affine:
                cur[0][:, 0], cur[1][:, 0], cur[2][:, 0] = VN, go + ge * d, VN
            else:
                cur[0][:, 0] = go * d
        if d <= N:  # column 0
            if affine:
                cur[0][:, d], cur[1][:, d], cur[2][:, d] = VN, VN, (0 if free_end else go + ge * d)
            else:
                cur[0][:, d] = go * d
        for p in np.flatnonzero(end_d == d):
            score[p] = max(int(x[p, ns[p]]) for x in cur)
        prev2, prev1 = prev1, cur
    return code, score


def _chooser(order):
    return [None] + [next(s for s in order if mask >> s & 1) for mask in range(1, 8)]


def _finish(route, walked, up, left, i, j):
    """the end of pyref's walks: the leading gap, unless the last move left through a tile's exact corner (quirk Q2)"""
    if walked:
        if (not up) and left:
            _emit(route, 2, i)
        elif up and (not left):
            _emit(route, 1, j)
    elif i == 0 and j > 0:
        _emit(route, 1, j)
    elif j == 0 and i > 0:
        _emit(route, 2, i)
    else:
        route.append([0, 0])
    route.reverse()
    return [(r, o) for r, o in route]


def _emit(route, op, run):
    if route and route[-1][1] == op:
        route[-1][0] += run
    else:
        route.append([run, op])


def _walk(kind, code, n, m, ci, cj, order):
    """pyref.affine's / pyref.const's walk in global coordinates, on the codes, under an order of preference.
    Returns (route, [(site, tied set, i, j)] of the tied argmaxes the walk consulted)."""
    ch = _chooser(order)
    ties, route = [], []
    i, j = n, m
    up = left = walked = False
    if kind == "const":
        while i > 0 and j > 0:
            walked = True
            mk = int(code[i, j]) & 7
            k = ch[mk]
            if mk in SET_NAME:
                ties.append(("V", SET_NAME[mk], i, j))
            _emit(route, k, 1)
            up = left = False
            if k != 1:
                up = (i - 1) % ci == 0
                i -= 1
            if k != 2:
                left = (j - 1) % cj == 0
                j -= 1
        return _finish(route, walked, up, left, i, j), ties
    k = 0
    if i > 0 and j > 0:
        mk = int(code[i, j]) >> 9
        k = ch[mk]
        if mk in SET_NAME:
            ties.append(("final", SET_NAME[mk], i, j))
    while i > 0 and j > 0:
        walked = True
        _emit(route, k, 1)
        mk = (int(code[i, j]) >> (3 * k)) & 7
        nk = ch[mk]
        i0, j0 = i, j
        up = left = False
        if k != 1:
            up = (i - 1) % ci == 0
            i -= 1
        if k != 2:
            left = (j - 1) % cj == 0
            j -= 1
        if i > 0 and j > 0:  # (at an edge the next state is never read: not a consulted argmax)
            if up:  # quirk Q1: the state restarts as the argmax at the entry cell, whatever the recurrence said
                mq = int(code[i, j]) >> 9
                nk = ch[mq]
                if mq in SET_NAME:
                    ties.append(("Q1", SET_NAME[mq], i, j))
            elif mk in SET_NAME:
                ties.append((SITE_NAME[k], SET_NAME[mk], i0, j0))
        k = nk
    return _finish(route, walked, up, left, i, j), ties


def walk_batch(mode, scores, go, ge, alphas, betas, checkers=(10000,), orders=(MID,)):
    """{(checkersize, order): [(score, route, ties) per pair]}: one fill per pair, one walk per checkerboard size and order.
    The high-memory modes and AffineGapLocal have no checkerboard: their walks are those of a checkerboard no pair reaches."""
    kind = kind_of(mode)
    sizes = [(len(a) + 1) * (len(b) + 1) for a, b in zip(alphas, betas)]
    assert min(len(a) for a in alphas) > 0 and min(len(b) for b in betas) > 0
    idx = sorted(range(len(alphas)), key=lambda p: sizes[p])
    out = {(cs, o): [None] * len(alphas) for cs in checkers for o in orders}
    at = 0
    while at < len(idx):
        grp, N, Mx = [], 0, 0
        while at < len(idx):
            p = idx[at]
            n2, m2 = max(N, len(alphas[p])), max(Mx, len(betas[p]))
            if grp and (len(grp) + 1) * (n2 + 1) * (m2 + 1) > CELL_LIMIT:
                break
            grp.append(p); N, Mx = n2, m2; at += 1
        code, score = _fill_chunk(kind, scores, go, ge if kind != "const" else 0, [alphas[p] for p in grp], [betas[p] for p in grp])
        for q, p in enumerate(grp):
            n, m = len(alphas[p]), len(betas[p])
            cp = np.ascontiguousarray(code[q, :n + 1, :m + 1])
            for cs in checkers:
                big = mode not in LOWMEM
                for o in orders:
                    route, ties = _walk(kind, cp, n, m, (1 << 60) if big else cs, (1 << 60) if big else cs, o)
                    out[(cs, o)][p] = (int(score[q]), route, ties)
        del code
    return out


def census(mode, scores, go, ge, alpha, beta, ci=10000, cj=10000, order=MID):
    """per pair a Counter {(site, tied set): cells} of the tied argmaxes the reference's walk consults (square checkerboards)"""
    assert ci == cj
    return [collections.Counter((s, t) for s, t, _, _ in ties) for _, _, ties in walk_batch(mode, scores, go, ge, alpha, beta, (ci,), (order,))[(ci, order)]]


def as_result(rows):
    """[(score, route, ...)] in the layout of oracle.align_batch"""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r[1]) for r in rows])
    ops = np.zeros(int(off[-1]), oracle.CIGAR_DTYPE)
    flat = [x for r in rows for x in r[1]]
    ops["run_length"] = [x[0] for x in flat]
    ops["op"] = [x[1] for x in flat]
    return np.asarray([r[0] for r in rows], np.int64), ops, off


def decided_otherwise(order, tset):
    """whether `order` takes another branch than tripleMaxTrace on a tied set ("MI", "MD", "ID", "MID")"""
    first = lambda o: next(s for s in o if SITE_NAME[s] in tset)
    return first(order) != first(MID)


# ---- the batches -------------------------------------------------------------------------------------------------------------------
def _source(rng, kind, length):
    if kind == 0:    # four letters
        return rng.integers(0, 4, size=length).astype(np.uint8)
    if kind == 1:    # two letters
        x, y = rng.choice(4, size=2, replace=False)
        return np.where(rng.random(length) < 0.5, x, y).astype(np.uint8)
    period = int(rng.integers(1, 5))  # tandem repeats of period 1 .. 4
    unit = rng.integers(0, 4, size=period)
    if period > 1 and len(set(unit.tolist())) == 1:
        unit[0] = (unit[0] + 1) % 4
    return np.resize(unit, length).astype(np.uint8)


def _pair(rng, k, n, m, sub, indel):
    """pair k of a batch, n x m: kind k % 3 (four letters, two letters, tandem repeat); one side a copy of the other with a few
    substitutions and indels, the shorter side cut from inside the longer one's span; in every other pair of a kind the two sides
    are exchanged (alpha the mutated copy), so that the D-site classes are reached as the I-site ones are"""
    kind, flip = k % 3, (k // 3) % 2
    length = max(n, m) + 24
    x = _source(rng, kind, length)
    y = common.mutate(rng, x, sub=sub, indel=indel * (1 if kind == 0 else 3), geo=0.5)  # (indels inside repeats are where the gap states tie)
    if len(y) < length:
        y = np.concatenate([y, _source(rng, kind, length - len(y))])
    sa, sb = (y, x) if flip else (x, y)
    if n <= m:
        off = int(rng.integers(0, m - n + 1))
        a, b = sa[off:off + n], sb[:m]
    else:
        off = int(rng.integers(0, n - m + 1))
        a, b = sa[:n], sb[off:off + m]
    return np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)


def _shaped(seed, shapes, sub=0.05, indel=0.04):
    rng = np.random.default_rng(seed)
    pairs = [_pair(rng, k, n, m, sub, indel) for k, (n, m) in enumerate(shapes)]
    return [a for a, _ in pairs], [b for _, b in pairs]


def _shapes(seed, count, n_lo, n_hi, m_lo, m_hi, fixed=()):
    rng = np.random.default_rng(seed)
    out = list(fixed)
    while len(out) < count:
        out.append((int(rng.integers(n_lo, n_hi + 1)), int(rng.integers(m_lo, m_hi + 1))))
    return out


def _reads(seed, count, n_lo, n_hi, sub, indel):
    """fast-path shapes: reads of n_lo .. n_hi bases in windows of 20 columns fewer to 40 more (with gaps this cheap a read spreads
    over a longer window in more runs than the walk stages; in a shorter one it has to delete), the block edges among the lengths"""
    rng = np.random.default_rng(seed)
    ns = [n_lo, n_hi, min(n_lo + 1, n_hi), n_hi - 1] + [int(x) for x in rng.integers(n_lo, n_hi + 1, size=count - 4)]
    return _shaped(seed + 1, [(n, max(1, n + int(rng.integers(-20, 41)))) for n in ns], sub=sub, indel=indel)


@functools.lru_cache(maxsize=None)
def batch(name):
    """(alphas, betas) of a named batch, in the shapes of asym.batch's routes; for xp* alpha is the window.  Shared: do not change them."""
    if name == "small":      # one strip
        return _shaped(8001, _shapes(8101, 30, 40, 150, 40, 190, fixed=((160, 160), (1, 30), (30, 1), (159, 400))))
    if name == "long16":     # several 160-row strips (128-row ones in the latency geometry)
        return _shaped(8002, _shapes(8102, 12, 170, 700, 200, 1100, fixed=((321, 330), (700, 1500))))
    if name == "tall12":     # tall: many strips, few columns
        rng = np.random.default_rng(8103)  # half of the pairs tall by hundreds of rows, half by only 10 .. 40: there an extra base of beta has to be inserted
        narrow = _shaped(8003, [(1300, 200)] + [(int(rng.integers(300, 1301)), int(rng.integers(100, 201))) for _ in range(5)], sub=0.08, indel=0.1)
        near = _shaped(8013, [(n, n - int(rng.integers(10, 41))) for n in (int(x) for x in rng.integers(300, 901, size=6))])
        return narrow[0] + near[0], narrow[1] + near[1]
    if name == "coop":       # beta >= 1024: pipelined strips, wave-cooperative traceback
        return _shaped(8004, _shapes(8104, 8, 600, 1000, 1024, 1300, fixed=((900, 1024), (100, 1500))))
    if name == "long40":     # the snapshot suites' shape
        return _shaped(8005, _shapes(8105, 24, 161, 700, 200, 1500, fixed=((700, 1500), (161, 700))))
    if name == "w64":        # two or more 640-row strips in at least a third of the pairs
        return _shaped(8006, [(1281, 1300), (2000, 1500), (1500, 1480), (1700, 900), (300, 1200), (641, 700), (900, 1400), (640, 1000), (1000, 640), (1290, 1285)])
    if name == "panels":     # row panels of two strips, at 16 and at 64 lanes
        return _shaped(8007, [(1400, 1450), (1700, 2600), (2700, 900), (3300, 3340)], sub=0.03, indel=0.03)
    if name in ("fp1", "fp2", "fp3"):
        k = int(name[2])
        return _reads(8010 + 2 * k, 24 if k == 3 else 36, 160 * (k - 1) + 1, 160 * k, sub=0.05 / k, indel=0.03 / k)
    if name in ("xp1", "xp2", "xp3"):  # target = window, query = read
        k = int(name[2])
        reads, wins = _reads(8020 + 2 * k, 24 if k == 3 else 36, 160 * (k - 1) + 1, 160 * k, sub=0.05 / k, indel=0.03 / k)
        return wins, reads
    if name == "diag":       # block_diag: three-block reads on a tandem repeat behind a unique head, one indel of whole periods
        rng = np.random.default_rng(8030)
        alphas, betas = [], []
        for k in range(12):
            n = [480, 479, 420, 421][k] if k < 4 else int(rng.integers(420, 481))  # (a top block of at least 100 rows: room for the head and the indel)
            period = 2 + k % 3
            unit = rng.permutation(4)[:period].astype(np.uint8)
            head = rng.integers(0, 4, size=int(rng.integers(20, n - 2 * 160 - 30))).astype(np.uint8)
            cut = period * int(rng.integers(1, 4))  # the indel: anywhere in the repeat it costs the same, and the preference for M takes it to the head
            flank = rng.integers(0, 4, size=int(rng.integers(0, 12))).astype(np.uint8)
            long_, short = np.concatenate([head, np.resize(unit, n + cut - len(head))]), np.concatenate([head, np.resize(unit, n - len(head))])
            read, win = (short, long_) if k % 2 else (np.concatenate([head, np.resize(unit, n - len(head))]), np.concatenate([head, np.resize(unit, n - cut - len(head))]))
            alphas.append(np.ascontiguousarray(read, np.uint8)); betas.append(np.ascontiguousarray(np.concatenate([flank, win]), np.uint8))
        return alphas, betas
    raise KeyError(name)


# the checkerboard sizes each batch is run with on the GPU (low-memory modes; 10000: beyond every pair)
CHECKERS = {"small": (7, 10000), "long16": (7, 10000), "long40": (3, 10000), "w64": (16, 10000), "panels": (1000, 10000), "fp2": (7, 10000)}
SMALL_CHECKERS = {"small": 7, "long16": 7, "long40": 3, "w64": 16, "fp2": 7}  # where quirk Q1 is reached
# batch -> (modes, affine sets, constant-gap sets): what tests/test_ties_gpu.py runs and tests/test_ties_cpu.py checks.  Every set costs
# a fill of every pair on the CPU, so the long batches take one set in which two gaps beat a mismatch and the one in which they equal it.
ALL_A, ALL_C = tuple(AFFINE_SETS), tuple(CONST_SETS)
PLAN = collections.OrderedDict([
    ("small", ((0, 1, 2, 3, 4), ALL_A, ALL_C)),
    ("long16", ((0, 1, 2, 3, 4), ("hc70", "hc3010", "tie15"), ("hc40", "tie15"))),
    ("tall12", ((0, 1, 2, 3, 4), ("hc70", "tie15"), ("hc70", "tie15"))),
    ("coop", ((0, 1, 2, 3, 4), ("hc70", "tie15"), ("hc40", "tie15"))),
    ("long40", ((0, 1, 2, 4), ("hc70", "tie15"), ("hc40", "tie15"))),
    ("w64", ((0, 1, 2, 4), ("hc70", "tie15"), ("hc70", "tie15"))),
    ("panels", ((0, 1, 2, 4), ("hc70", "tie15"), ("hc40", "tie15"))),
    ("fp1", ((0,), ALL_A, ())), ("fp2", ((0,), ("hc70", "hc3010", "tie15"), ())), ("fp3", ((0,), ("hc70", "tie15"), ())),
    ("xp1", ((3,), ALL_A, ())), ("xp2", ((3,), ("hc70", "hc3010", "tie15"), ())), ("xp3", ((3,), ("hc70", "tie15"), ())),
    ("diag", ((0,), ("tie15",), ())),
])


def plan_sets(name, mode):
    modes, aff, con = PLAN[name]
    assert mode in modes, (name, mode)
    return aff if mode in AFFINE_MODES else con


def checkers(name, mode):
    return CHECKERS.get(name, (10000,)) if mode in LOWMEM else (10000,)


@functools.lru_cache(maxsize=None)
def _runs(name, kind, sname, lowmem):
    """every walk of a batch under one set: {(checkersize, order): [(score, route, ties)]}"""
    mode = {"affine": 0 if lowmem else 2, "local": 3, "const": 1 if lowmem else 4}[kind]
    table, go, ge = params(mode, sname)
    alphas, betas = batch(name)
    return walk_batch(mode, table, go, ge, alphas, betas, checkers(name, mode), ORDERS if sname != "control" else (MID, MDI))


def runs(name, mode, sname, ci=10000, order=MID):
    """(a low-memory mode beyond every checkerboard edge walks as its high-memory twin: one fill and one set of walks for both)"""
    kind = kind_of(mode)
    return _runs(name, kind, sname, kind != "local" and name in CHECKERS)[(ci, order)]


def counts(name, mode, sname, ci=10000):
    return [collections.Counter((s, t) for s, t, _, _ in ties) for _, _, ties in runs(name, mode, sname, ci)]


@functools.lru_cache(maxsize=None)
def expected(name, mode, sname, ci=10000):
    """the oracle's (scores, ops, offsets): computed once, shared by every route that must reproduce it"""
    table, go, ge = params(mode, sname)
    alphas, betas = batch(name)
    return oracle.align_batch(mode, table, go, ge, alphas, betas, ci, ci, threads=8)


def changed(name, mode, sname, order, ci=10000):
    """per pair: does the walk under `order` give another CIGAR than the walk under (M, I, D)"""
    return [r[1] != q[1] for r, q in zip(runs(name, mode, sname, ci, order), runs(name, mode, sname, ci))]


# ---- the conditions ----------------------------------------------------------------------------------------------------------------
# The classes a batch must reach (at least MIN_PAIRS pairs, MIN_CELLS cells over the batch).  No set reaches every class, for reasons
# of arithmetic: each set is asked for what its relation between the penalties produces (NOT_REQUIRED has the reasons, DESIGN.md 4.32
# the counts), and the sets of a batch must ask for the whole table between them (tests/test_ties_cpu.py).
MIN_PAIRS, MIN_CELLS = 3, 10
REQUIRED = [("M", "MI"), ("M", "MD"), ("M", "ID"), ("M", "MID"), ("I", "MI"), ("I", "MD"), ("I", "ID"), ("D", "MD")]
REQUIRED_Q1 = [("Q1", "MI"), ("Q1", "MD"), ("Q1", "ID")]
REQUIRED_CONST = [("V", "MI"), ("V", "MD"), ("V", "ID"), ("V", "MID")]
# EXEMPT: (batch, kind, set) -> the classes that batch does not reach under that set (fewer than MIN_PAIRS pairs or MIN_CELLS cells at
# one of its checkerboard sizes), taken from the census; every other class of the table is required there.  tests/test_ties_cpu.py
# fails when an entry is stale -- the class does meet the bound -- and when the sets of a batch do not require the whole table between
# them.  Why a class stays out of reach:
#   hc70, hc40, hc3010 (two gaps BEAT every mismatch): "MID" at M, V and Q1 asks match + h(i-2, j-2) = h(i-1, j-2) + e = h(i-2, j-1) + e, both
#     neighbours a whole match and a gap above the diagonal cell: a few cells in a few pairs.  It is what the tie table is for;
#   hc3010 (gapOpen < 0): a tie in the I or D recurrence asks M + gapOpen = I (or D) exactly; reached where the match scores 90 and
#     100 happen to differ by gapExtend, so in few cells of the shorter batches;
#   tie15 (two gaps EQUAL a mismatch): wherever I and D tie after a substitution M ties with them: "MID" takes the place of "ID" at M, V
#     and Q1, and the I site's "MD" and "ID", which need a D candidate above M's, do not occur at all (0 cells in every batch).
EXEMPT = {
    ('small', 'affine', 'hc70'): (('M', 'MID'),),
    ('small', 'affine', 'hc3010'): (('M', 'MID'), ('Q1', 'ID')),
    ('small', 'affine', 'hc40'): (('M', 'MID'),),
    ('small', 'affine', 'tie15'): (('M', 'ID'), ('I', 'MD'), ('I', 'ID'), ('Q1', 'ID')),
    ('small', 'const', 'hc40'): (('V', 'MID'),),
    ('small', 'const', 'hc70'): (('V', 'MID'),),
    ('small', 'const', 'tie15'): (('V', 'ID'),),
    ('small', 'local', 'hc70'): (('M', 'MID'),),
    ('small', 'local', 'hc3010'): (('M', 'MID'), ('D', 'MD')),
    ('small', 'local', 'hc40'): (('M', 'MID'),),
    ('small', 'local', 'tie15'): (('M', 'ID'), ('I', 'MD'), ('I', 'ID')),
    ('long16', 'affine', 'hc70'): (('M', 'MID'),),
    ('long16', 'affine', 'hc3010'): (('M', 'MID'), ('D', 'MD')),
    ('long16', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID'), ('Q1', 'ID')),
    ('long16', 'local', 'hc70'): (('M', 'MID'),),
    ('long16', 'local', 'hc3010'): (('M', 'MID'),),
    ('long16', 'local', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('tall12', 'affine', 'hc70'): (('M', 'MID'),),
    ('tall12', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('tall12', 'const', 'hc70'): (('V', 'MID'),),
    ('tall12', 'local', 'hc70'): (('M', 'MID'),),
    ('tall12', 'local', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('coop', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('coop', 'local', 'hc70'): (('M', 'MID'),),
    ('coop', 'local', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('long40', 'affine', 'hc70'): (('M', 'MID'),),
    ('long40', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('long40', 'const', 'hc40'): (('V', 'MID'),),
    ('w64', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID'), ('Q1', 'ID')),
    ('panels', 'affine', 'hc70'): (('M', 'MID'),),
    ('panels', 'affine', 'tie15'): (('M', 'ID'), ('I', 'MD'), ('I', 'ID')),
    ('panels', 'const', 'hc40'): (('V', 'MID'),),
    ('panels', 'const', 'tie15'): (('V', 'ID'),),
    ('fp1', 'affine', 'hc70'): (('M', 'MID'),),
    ('fp1', 'affine', 'hc3010'): (('M', 'MID'),),
    ('fp1', 'affine', 'hc40'): (('M', 'MID'),),
    ('fp1', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('fp2', 'affine', 'hc70'): (('M', 'MID'),),
    ('fp2', 'affine', 'hc3010'): (('M', 'MID'), ('I', 'ID'), ('D', 'MD')),
    ('fp2', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID'), ('Q1', 'ID')),
    ('fp3', 'affine', 'hc70'): (('M', 'MID'),),
    ('fp3', 'affine', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('xp1', 'local', 'hc70'): (('M', 'MID'),),
    ('xp1', 'local', 'hc3010'): (('M', 'MID'), ('I', 'MI'), ('I', 'ID'), ('D', 'MD')),
    ('xp1', 'local', 'hc40'): (('M', 'MID'),),
    ('xp1', 'local', 'tie15'): (('M', 'ID'), ('I', 'MD'), ('I', 'ID')),
    ('xp2', 'local', 'hc70'): (('M', 'MID'),),
    ('xp2', 'local', 'hc3010'): (('M', 'MID'), ('I', 'MI'), ('I', 'ID'), ('D', 'MD')),
    ('xp2', 'local', 'tie15'): (('I', 'MD'), ('I', 'ID')),
    ('xp3', 'local', 'tie15'): (('I', 'MD'), ('I', 'ID')),
}
ALSO_REQUIRED = {"tie15": [("Q1", "MID")]}


def family_table(mode):
    """what the sets of a batch must require between them: the whole table"""
    return REQUIRED if mode in AFFINE_MODES else REQUIRED_CONST


def full_table(name, mode, sname, ci=10000):
    if mode not in AFFINE_MODES:
        return list(REQUIRED_CONST)
    req = list(REQUIRED)
    if mode in LOWMEM and ci == SMALL_CHECKERS.get(name):
        req += REQUIRED_Q1 + ALSO_REQUIRED.get(sname, [])
    return req


def required(name, mode, sname, ci=10000):
    skip = EXEMPT.get((name, kind_of(mode), sname), ())
    return [c for c in full_table(name, mode, sname, ci) if c not in skip]


def reaches(cnts, cls):
    return sum(1 for c in cnts if c[cls]) >= MIN_PAIRS and sum(c[cls] for c in cnts) >= MIN_CELLS


def has_id(cnt):
    """a tie with I and D both in the tied set, at any site"""
    return any(v and t in ("ID", "MID") for (_, t), v in cnt.items())


@functools.lru_cache(maxsize=None)
def decisive(name, mode, sname, ci=10000):
    """The condition that keeps a batch from passing vacuously, on the census of the reference's route alone: a tie with I and D both
    in the tied set on the route of at least half of the pairs, every required class on at least MIN_PAIRS pairs and MIN_CELLS cells,
    a tied final state on at least one pair (affine), and the census' own walk equal to the oracle.  Raises; returns True."""
    cnts = counts(name, mode, sname, ci)
    common.assert_same(as_result(runs(name, mode, sname, ci)), expected(name, mode, sname, ci), "census walk against the oracle: %s mode %d %s checkersize %d" % (name, mode, sname, ci))
    frac = sum(has_id(c) for c in cnts) / len(cnts)
    assert frac >= 0.5, "only %.2f of the pairs of %s have an I/D tie on their route (mode %d, %s, checkersize %d)" % (frac, name, mode, sname, ci)
    for cls in required(name, mode, sname, ci):
        pairs, cells = sum(1 for c in cnts if c[cls]), sum(c[cls] for c in cnts)
        assert pairs >= MIN_PAIRS and cells >= MIN_CELLS, "class %s %s: %d pairs, %d cells in %s (mode %d, %s, checkersize %d)" % (cls + (pairs, cells, name, mode, sname, ci))
    if mode in AFFINE_MODES:
        assert any(c[("final", t)] for c in cnts for t in SET_NAME.values()), "no tied final state in %s (mode %d, %s)" % (name, mode, sname)
    return True


def table_row(name, mode, sname, ci=10000):
    """the census of a batch as {class: (pairs, cells)}, for DESIGN.md's table"""
    cnts = counts(name, mode, sname, ci)
    keys = sorted({k for c in cnts for k in c})
    return collections.OrderedDict((k, (sum(1 for c in cnts if c[k]), sum(c[k] for c in cnts))) for k in keys)


def staged(name, mode, sname, ci=10000):
    """the fast path's own condition: by the oracle's run counts at most half of the pairs exceed the 64 runs the walk stages (those
    are aligned again on the general path), and the pairs that stay still have an I/D tie on at least half of their routes"""
    runs_ = np.diff(expected(name, mode, sname, ci)[2])
    cnts = counts(name, mode, sname, ci)
    keep = [c for c, r in zip(cnts, runs_) if r <= 64]
    assert 2 * len(keep) >= len(cnts), "%d of %d CIGARs of %s (%s) exceed 64 runs" % (len(cnts) - len(keep), len(cnts), name, sname)
    assert 2 * sum(has_id(c) for c in keep) >= len(keep), (name, sname)
    return True


def _m_run_over(route, lo, hi):
    """whether one ColM run of the CIGAR covers the rows lo + 1 .. hi: the route crosses them on a plain diagonal"""
    i = 0
    for run, op in route:
        if op == 0 and i <= lo and i + run >= hi:
            return True
        if op != 1:
            i += run
    return False


def _gap_inside(route, hi):
    """whether a gap run of the CIGAR starts on a row 1 .. hi behind a ColM run: an indel inside those rows, not a leading gap"""
    i, seen_m = 0, False
    for run, op in route:
        if op == 0:
            seen_m = True
        elif seen_m and 1 <= i <= hi:
            return True
        if op != 1:
            i += run
    return False


@functools.lru_cache(maxsize=None)
def diag_condition(sname="tie15", block=160):
    """the block_diag batch: in at least half of the pairs (1) the oracle's route holds an indel inside the top row block, so that no
    whole-read diagonal can finish the walk before block_diag is asked; (2) it crosses the middle row block (rows n - 2 * 160 + 1 ..
    n - 160) inside one ColM run; (3) the census shows, at the M site of a cell of that block, an MI or MD tie -- a co-optimal route
    with the gap inside the skipped block, which only the preference for M rules out.  The walk equals the oracle.  Returns the pairs that do."""
    rows = runs("diag", 0, sname)
    common.assert_same(as_result(rows), expected("diag", 0, sname), "census walk against the oracle: diag")
    good = []
    for p, ((_, route, ties), a) in enumerate(zip(rows, batch("diag")[0])):
        n = len(a)
        lo, hi = n - 2 * block, n - block
        inside = [t for t in ties if t[0] == "M" and t[1] in ("MI", "MD") and lo < t[2] <= hi]
        if lo >= 1 and _gap_inside(route, lo) and _m_run_over(route, lo, hi) and inside:
            good.append(p)
    assert 2 * len(good) >= len(rows), good
    return tuple(good)


def blind(name, mode, ci=10000):
    """the control: the fraction of the pairs of a batch whose route, under the penalties the route suites use, holds NO tie with I and D
    both in the tied set -- what those suites could not see"""
    cnts = counts(name, mode, "control", ci)
    return sum(not has_id(c) for c in cnts) / len(cnts)
