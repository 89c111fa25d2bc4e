"""Host-side mirror of the reference's `align` package API for the DP hot path.

Same names, argument meaning and error behaviour as the Go functions, so tests read like the
reference's own (/root/reference/align/affineGap_test.go, view_test.go):

  AffineGap, AffineGap_customizeCheckersize      /root/reference/align/affineGap.go:59,73
  ConstGap, ConstGap_customizeCheckersize        /root/reference/align/constGap.go:13,73
  AffineGap_highMem, AffineGapLocal              /root/reference/align/affineGap_highMem.go:99,105
  ConstGap_highMem                               /root/reference/align/constGap_highMem.go:11
  GoAffineGapLocalEngine, TargetQueryPair        /root/reference/align/affineGap_highMem.go:109-125
  View, PrintCigar                               /root/reference/align/view.go:26-60
  Cigar, ColM/ColI/ColD, the four score matrices /root/reference/align/align.go:12-64

Every alignment call goes through the C ABI into the HIP kernels (gonomics_amd/_lib.py); a single
pair is a batch of one.  Go panics map to exceptions: base >= 5 -> IndexError (index out of range),
empty input to a low-memory function (the Go code never terminates) -> ValueError.
"""
import os
from collections import namedtuple

import numpy as np

from . import _lib
from . import dna

ColM, ColI, ColD = 0, 1, 2
Cigar = namedtuple("Cigar", ["RunLength", "Op"])

DefaultScoreMatrix = [
    [91, -114, -31, -123, -44],
    [-114, 100, -125, -31, -43],
    [-31, -125, 100, -114, -43],
    [-123, -31, -114, 91, -44],
    [-44, -43, -43, -44, -43],
]
HoxD55ScoreMatrix = [
    [91, -114, -31, -123, 0],
    [-114, 100, -125, -31, 0],
    [-31, -125, 100, -114, 0],
    [-123, -31, -114, 91, 0],
    [0, 0, 0, 0, 0],
]
MouseRatScoreMatrix = [row[:] for row in HoxD55ScoreMatrix]
HumanChimpTwoScoreMatrix = [
    [90, -330, -236, -356, -208],
    [-330, 100, -318, -236, -196],
    [-236, -318, 100, -330, -196],
    [-356, -236, -330, 90, -208],
    [-208, -196, -196, -208, -202],
]


def _raise(e):
    if e.code == _lib.GNX_EBASE:
        raise IndexError("runtime error: index out of range (dna.Base >= 5 used as a score-matrix index)") from e
    if e.code == _lib.GNX_EEMPTY:
        raise ValueError("empty sequence: the reference's checkerboard loop never terminates on it") from e
    raise e


def _to_route(ops):
    return [Cigar(int(r), int(o)) for r, o in zip(ops["run_length"], ops["op"])]


def _one(params, alpha, beta):
    try:
        score, ops = _lib.align_pair(params, alpha, beta)
    except _lib.GnxError as e:
        _raise(e)
    return score, _to_route(ops)


def AffineGap(alpha, beta, scores, gapOpen, gapExtend):
    return AffineGap_customizeCheckersize(alpha, beta, scores, gapOpen, gapExtend, 10000, 10000)


def AffineGap_customizeCheckersize(alpha, beta, scores, gapOpen, gapExtend, checkersize_i, checkersize_j):
    return _one(_lib.make_params(_lib.GNX_AFFINE_GAP, scores, gapOpen, gapExtend, checkersize_i, checkersize_j), alpha, beta)


def ConstGap(alpha, beta, scores, gapPen):
    return ConstGap_customizeCheckersize(alpha, beta, scores, gapPen, 10000, 10000)


def ConstGap_customizeCheckersize(alpha, beta, scores, gapPen, checkersize_i, checkersize_j):
    return _one(_lib.make_params(_lib.GNX_CONST_GAP, scores, gapPen, 0, checkersize_i, checkersize_j), alpha, beta)


def AffineGap_highMem(alpha, beta, scores, gapOpen, gapExtend):
    return _one(_lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend), alpha, beta)


def AffineGapLocal(target, query, scores, gapOpen, gapExtend):
    return _one(_lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend), target, query)


def ConstGap_highMem(alpha, beta, scores, gapPen):
    return _one(_lib.make_params(_lib.GNX_CONST_GAP_HIGHMEM, scores, gapPen), alpha, beta)


def AlignBatch(params, alphas, betas):
    """Batched form used by loops over independent pairs (cmd/globalAlignmentAnchor.go:352-384).
    Returns [(score, route), ...] in input order."""
    try:
        scores, ops, off = _lib.align_batch(params, alphas, betas)
    except _lib.GnxError as e:
        _raise(e)
    return [(int(scores[k]), _to_route(ops[off[k]:off[k + 1]])) for k in range(len(alphas))]


# ---- score-only calls (gnx_score_*: an extension, no Go function returns a score alone) ------------------------------------------
def ScoreBatch(params, alphas, betas):
    """The scores AlignBatch would return for these pairs, without their routes.  Returns [score, ...] in input order."""
    try:
        scores = _lib.score_batch(params, alphas, betas)
    except _lib.GnxError as e:
        _raise(e)
    return [int(x) for x in scores]


def _one_score(params, alpha, beta):
    return ScoreBatch(params, [alpha], [beta])[0]


def AffineGapScore(alpha, beta, scores, gapOpen, gapExtend):
    return _one_score(_lib.make_params(_lib.GNX_AFFINE_GAP, scores, gapOpen, gapExtend), alpha, beta)


def ConstGapScore(alpha, beta, scores, gapPen):
    return _one_score(_lib.make_params(_lib.GNX_CONST_GAP, scores, gapPen), alpha, beta)


def AffineGapLocalScore(target, query, scores, gapOpen, gapExtend):
    return _one_score(_lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend), target, query)


# ---- locate calls (gnx_locate_*): where in the target a query ends, without a route ------------------------------------------------
def LocateBatch(params, targets, queries):
    """AffineGapLocal's score and target end for every (target, query) pair: ([score, ...], [targetEnd, ...]) in input order.
    targetEnd = len(target) minus the trailing ColD run of the route AffineGapLocal returns: the target position just after the
    last aligned column.  params.mode must be GNX_AFFINE_GAP_LOCAL."""
    try:
        scores, ends = _lib.locate_batch(params, targets, queries)
    except _lib.GnxError as e:
        _raise(e)
    return [int(x) for x in scores], [int(x) for x in ends]


def AffineGapLocalEnd(target, query, scores, gapOpen, gapExtend):
    """(score, targetEnd) of AffineGapLocal(target, query, ...) without its route."""
    sc, ends = LocateBatch(_lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend), [target], [query])
    return sc[0], ends[0]


def LocateSpanBatch(params, targets, queries):
    """AffineGapLocal's score, target start and target end for every (target, query) pair: ([score, ...], [targetStart, ...],
    [targetEnd, ...]) in input order.  targetStart = the leading ColD run of the route AffineGapLocal returns (0 if it does not begin
    with one): the leftmost aligned target position; targetEnd as in LocateBatch.  params.mode must be GNX_AFFINE_GAP_LOCAL."""
    try:
        scores, starts, ends = _lib.locate_span_batch(params, targets, queries)
    except _lib.GnxError as e:
        _raise(e)
    return [int(x) for x in scores], [int(x) for x in starts], [int(x) for x in ends]


def AffineGapLocalSpan(target, query, scores, gapOpen, gapExtend):
    """(score, targetStart, targetEnd) of AffineGapLocal(target, query, ...) without its route."""
    sc, starts, ends = LocateSpanBatch(_lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend), [target], [query])
    return sc[0], starts[0], ends[0]


def ScoreAllPairs(seqs, params):
    """Scores of all x < y pairs of `seqs` from one device call: {(x, y): score} (what a distance matrix or the choice of the
    nearest pair of a progressive-alignment round needs)."""
    idx = [(x, y) for x in range(len(seqs)) for y in range(x + 1, len(seqs))]
    sc = ScoreBatch(params, [seqs[x] for x, _ in idx], [seqs[y] for _, y in idx]) if idx else []
    return {xy: s for xy, s in zip(idx, sc)}


def _first_maxima(scores, counts):
    """Per read the index of the FIRST maximum among its counts[r] consecutive scores (ties go to the lowest index)."""
    best, at = [], 0
    for k in counts:
        if k < 1:
            raise ValueError("a read without candidates")
        b = 0
        for c in range(1, k):
            if scores[at + c] > scores[at + b]:
                b = c
        best.append(b)
        at += k
    return best


def AlignBestOf(params, reads, candidates):
    """Best of K: candidates[r] is a list of K_r target sequences, or of (start, len) windows of the resident reference
    (_lib.set_reference).  One score call over all read x candidate pairs, per read the first maximum in candidate order, then one
    ordinary align call for the winners only.  Returns [(best_index, score, route), ...]: score and route are what AlignBatch gives
    for the winning pair."""
    if not reads:
        return []
    counts = [len(c) for c in candidates]
    flat = [c for cs in candidates for c in cs]
    windows = bool(flat) and isinstance(flat[0], tuple)
    rep = [reads[r] for r, k in enumerate(counts) for _ in range(k)]
    try:
        if windows:
            a_cat, a_off = _lib._cat(rep)
            sc = _lib.score_batch_by_offset(params, a_cat, a_off, [w[0] for w in flat], [w[1] for w in flat])
        else:
            sc = _lib.score_batch(params, rep, flat)
        best = _first_maxima(sc, counts)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
        win = [flat[int(first[r]) + b] for r, b in enumerate(best)]
        if windows:
            a_cat, a_off = _lib._cat(list(reads))
            scores, ops, off = _lib.align_batch_by_offset(params, a_cat, a_off, [w[0] for w in win], [w[1] for w in win])
        else:
            scores, ops, off = _lib.align_batch(params, list(reads), win)
    except _lib.GnxError as e:
        _raise(e)
    return [(best[r], int(scores[r]), _to_route(ops[off[r]:off[r + 1]])) for r in range(len(reads))]


def MapBestOf(params, reads, candidates, cigar=True):
    """Best of K on both strands in ONE device call (gnx_best_of_*): candidates[r] is a list of (start, len, strand) windows of the
    resident reference (_lib.set_reference), or of (target_bases, strand); strand 1 = the read's reverse complement.  Global modes
    align the read (alpha) to the window (beta); GNX_AFFINE_GAP_LOCAL aligns the read as the query to the window as the target.
    Returns [(best_index, score, route_or_None, target_end_or_None, cand_scores), ...]: per read the first maximum in candidate
    order with the score and route AlignBatch gives for that pair (route None with cigar=False), the target end in local mode, and
    every candidate's score.  A read without candidates gets (-1, 0, [] or None, 0 or None, [])."""
    if not reads:
        return []
    counts = [len(c) for c in candidates]
    flat = [c for cs in candidates for c in cs]
    resident = bool(flat) and len(flat[0]) == 3
    r_cat, r_off = _lib._cat(list(reads))
    c_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    try:
        if resident or not flat:
            args = ([w[0] for w in flat], [w[1] for w in flat], [w[2] for w in flat])
            out = _lib.best_of_by_offset(params, r_cat, r_off, c_off, *args, cigar=cigar) if flat else \
                _lib.best_of_windows(params, r_cat, r_off, np.zeros(1, np.uint8), c_off, [], [], [], cigar=cigar)
        else:
            t_cat, t_off = _lib._cat([w[0] for w in flat])
            out = _lib.best_of_windows(params, r_cat, r_off, t_cat[:-1], c_off, t_off[:-1], np.diff(t_off), [w[1] for w in flat], cigar=cigar)
    except _lib.GnxError as e:
        _raise(e)
    best, scores, ends, cand, ops, off = out
    return [(int(best[r]), int(scores[r]), _to_route(ops[off[r]:off[r + 1]]) if cigar else None, int(ends[r]) if ends is not None else None,
             [int(x) for x in cand[c_off[r]:c_off[r + 1]]]) for r in range(len(reads))]


# defaults of the seed vote (measured on 150-base reads with the C2 error model against a 16-mer index of every position)
SEED_VOTE_DEFAULTS = {"max_occ": 64, "bin": 32, "pad": 16, "max_cand": 4, "min_votes": 2}


def ReferenceIndexBuild(seedLen, seedStep=1):
    """gnx_reference_index_build: the k-mer index of the resident reference (_lib.set_reference), built and kept on the device."""
    try:
        _lib.reference_index_build(seedLen, seedStep)
    except _lib.GnxError as e:
        _raise(e)


def _vote_opts(vote_opts):
    opts = dict(SEED_VOTE_DEFAULTS)
    for k in vote_opts:
        if k not in opts:
            raise TypeError("unknown seed vote option %r" % k)
    opts.update(vote_opts)
    return opts


def SeedCandidates(reads, **vote_opts):
    """gnx_seed_candidates: per read its candidate windows of the resident reference by seed votes,
    [[(start, len, strand, votes), ...], ...] -- votes descending, then strand, then diagonal bin."""
    r_cat, r_off = _lib._cat(list(reads))
    try:
        off, start, ln, strand, votes = _lib.seed_candidates(r_cat, r_off, **_vote_opts(vote_opts))
    except _lib.GnxError as e:
        _raise(e)
    return [[(int(start[c]), int(ln[c]), int(strand[c]), int(votes[c])) for c in range(off[r], off[r + 1])] for r in range(len(reads))]


def MapReads(params, reads, cigar=True, **vote_opts):
    """Reads in, placements out: gnx_seed_candidates, then gnx_best_of_by_offset on its tables unchanged.  Returns MapBestOf's tuples
    plus the winner's absolute window start (None without a candidate): (best_index, score, route_or_None, target_end_or_None,
    cand_scores, window_start).  In GNX_AFFINE_GAP_LOCAL window_start + target_end is the reference position behind the alignment."""
    if not reads:
        return []
    r_cat, r_off = _lib._cat(list(reads))
    try:
        c_off, start, ln, strand, _ = _lib.seed_candidates(r_cat, r_off, **_vote_opts(vote_opts))
        best, scores, ends, cand, ops, off = _lib.best_of_by_offset(params, r_cat, r_off, c_off, start, ln, strand, cigar=cigar)
    except _lib.GnxError as e:
        _raise(e)
    return [(int(best[r]), int(scores[r]), _to_route(ops[off[r]:off[r + 1]]) if cigar else None, int(ends[r]) if ends is not None else None,
             [int(x) for x in cand[c_off[r]:c_off[r + 1]]], int(start[c_off[r] + best[r]]) if best[r] >= 0 else None) for r in range(len(reads))]


def _pair_result(out, n, c_off, w_start, cigar):
    """(per read, per pair) of MapBestPair / MapReadPairs from _lib.best_pair_*'s dict; w_start = every candidate's window start"""
    per_read = []
    for r in range(n):
        b = int(out["best"][r])
        at = int(w_start[c_off[r] + b]) if b >= 0 else None
        per_read.append((b, int(out["score"][r]), _to_route(out["ops"][out["off"][r]:out["off"][r + 1]]) if cigar else None, int(out["target_end"][r]),
                         [int(x) for x in out["cand_score"][c_off[r]:c_off[r + 1]]],
                         at + int(out["target_start"][r]) if b >= 0 else None, at + int(out["target_end"][r]) if b >= 0 else None,
                         int(out["second_score"][r]) if out["second_score"][r] != np.iinfo(np.int64).min else None))
    return per_read, [(bool(out["proper"][k]), int(out["tlen"][k])) for k in range(n // 2)]


def MapBestPair(params, reads, candidates, min_insert, max_insert, unpaired_penalty=0, cigar=True, target=None):
    """Best proper pair in ONE device call (gnx_best_pair_*): reads[2k] and reads[2k + 1] are mates, candidates[r] a list of (start, len,
    strand) windows of the resident reference (_lib.set_reference) or, with target given, of that sequence; strand 1 = the read's reverse
    complement; the mode GNX_AFFINE_GAP_LOCAL.  The two mates are chosen together: opposite strands, the forward one first, min_insert <=
    outer distance <= max_insert; the best such combination wins unless the two separate first maxima beat it by more than
    unpaired_penalty (include/gnx_align.h states the rule).  Returns (per_read, per_pair): per read MapBestOf's tuple plus (abs_start,
    abs_end, second_score) -- the alignment's span in the coordinates of the window starts (None without a candidate) and the best score
    among the read's other candidates (None without one); per pair (proper, tlen)."""
    if len(reads) % 2:
        raise ValueError("MapBestPair: reads come in mate pairs (an even number)")
    if not reads:
        return [], []
    flat = [c for cs in candidates for c in cs]
    r_cat, r_off = _lib._cat(list(reads))
    c_off = np.concatenate([[0], np.cumsum([len(c) for c in candidates])]).astype(np.int64)
    opts = _lib.pair_opts(min_insert, max_insert, unpaired_penalty)
    w_start = np.array([w[0] for w in flat], dtype=np.int64)
    args = (c_off, w_start, [w[1] for w in flat], [w[2] for w in flat])
    try:
        if target is None and flat:
            out = _lib.best_pair_by_offset(params, opts, r_cat, r_off, *args, cigar=cigar)
        else:
            out = _lib.best_pair_windows(params, opts, r_cat, r_off, np.zeros(1, np.uint8) if target is None else target, *args, cigar=cigar)
    except _lib.GnxError as e:
        _raise(e)
    return _pair_result(out, len(reads), c_off, w_start, cigar)


def MapReadPairs(params, reads, min_insert, max_insert, unpaired_penalty=0, cigar=True, **vote_opts):
    """Mate pairs in, placements out: gnx_seed_candidates over all mates, then gnx_best_pair_by_offset on its tables unchanged.  Returns
    what MapBestPair returns; abs_start / abs_end are positions of the resident reference."""
    if len(reads) % 2:
        raise ValueError("MapReadPairs: reads come in mate pairs (an even number)")
    if not reads:
        return [], []
    r_cat, r_off = _lib._cat(list(reads))
    try:
        c_off, start, ln, strand, _ = _lib.seed_candidates(r_cat, r_off, **_vote_opts(vote_opts))
        out = _lib.best_pair_by_offset(params, _lib.pair_opts(min_insert, max_insert, unpaired_penalty), r_cat, r_off, c_off, start, ln, strand, cigar=cigar)
    except _lib.GnxError as e:
        _raise(e)
    return _pair_result(out, len(reads), c_off, start, cigar)


# ---- alignment summaries (gnx_summarize_*): identity, edit distance, the =/X CIGAR and the column re-score of finished alignments ----
ColEq, ColX = _lib.GNX_XCOL_EQ, _lib.GNX_XCOL_X


def _routes_to_ops(routes):
    off = np.zeros(len(routes) + 1, dtype=np.int64)
    if routes:
        off[1:] = np.cumsum([len(r) for r in routes])
    ops = np.zeros(int(off[-1]), dtype=_lib.CIGAR_DTYPE)
    flat = [c for r in routes for c in r]
    if flat:
        ops["run_length"] = [c[0] for c in flat]
        ops["op"] = [c[1] for c in flat]
    return ops, off


def _summary_dicts(out, xops, xoff):
    res = []
    for k in range(out.shape[0]):
        d = {f: int(out[f][k]) for f in _lib.SUMMARY_FIELDS}
        if xops is not None:
            d["xcigar"] = _to_route(xops[xoff[k]:xoff[k + 1]])
        res.append(d)
    return res


def Summarize(params, alphas, betas, routes, xcigar=False):
    """What is IN finished alignments (gnx_summarize_batch): routes[k] is the CIGAR of alphas[k] against betas[k] (a list of Cigar, as
    AlignBatch returns it).  Returns one dict per pair with gnx_aln_summary's fields -- rescore, alpha_used, beta_used, alpha_start,
    alpha_end, n_equal, n_mismatch, ins_bases, del_bases, gap_runs, n_xops (include/gnx_align.h defines each) -- plus "xcigar", the =/X
    form of the route (ops ColEq / ColX in place of ColM), with xcigar=True."""
    if not routes:
        return []
    ops, off = _routes_to_ops(routes)
    try:
        out, xops, xoff = _lib.summarize_batch(params, alphas, betas, ops, off, xcigar=xcigar)
    except _lib.GnxError as e:
        _raise(e)
    return _summary_dicts(out, xops, xoff)


def SummarizeByOffset(params, reads, windows, routes, xcigar=False):
    """Summarize against the resident reference (gnx_summarize_batch_by_offset): windows[k] = (start, len), reads[k] in the orientation
    it was aligned in (a strand-1 winner: dna.ReverseComplement of the read).  The roles are MapBestOf's: global modes read = alpha,
    window = beta; GNX_AFFINE_GAP_LOCAL window = alpha (the target), read = beta."""
    if not routes:
        return []
    ops, off = _routes_to_ops(routes)
    r_cat, r_off = _lib._cat(list(reads))
    try:
        out, xops, xoff = _lib.summarize_batch_by_offset(params, r_cat, r_off, [w[0] for w in windows], [w[1] for w in windows], ops, off, xcigar=xcigar)
    except _lib.GnxError as e:
        _raise(e)
    return _summary_dicts(out, xops, xoff)


def FormatXCigar(route):
    """An extended route as text, e.g. "12=1X30=2D5=" ("*" for an empty one)"""
    runes = {ColM: "M", ColI: "I", ColD: "D", ColEq: "=", ColX: "X"}
    return "".join("%d%s" % (c[0], runes[c[1]]) for c in route) or "*"


def MDTags(params, alphas, betas, routes):
    """The MD string of every alignment (gnx_md_batch): routes[k] is the CIGAR of alphas[k] against betas[k], and alphas[k] is the
    DESCRIBED side -- the reference of SAM's MD:Z tag -- whose letters stand under every substitution and deletion, e.g. "3T2^G3".
    include/gnx_align.h defines the string; in GNX_AFFINE_GAP_LOCAL the free end gaps are outside it."""
    if not routes:
        return []
    ops, off = _routes_to_ops(routes)
    try:
        md, md_off = _lib.md_batch(params, alphas, betas, ops, off)
    except _lib.GnxError as e:
        _raise(e)
    return _lib.md_strings(md, md_off)


def MDTagsByOffset(params, reads, windows, routes):
    """MDTags against the resident reference (gnx_md_batch_by_offset): windows[k] = (start, len) is the described side, reads[k] the
    query in the orientation it was aligned in.  GNX_AFFINE_GAP_LOCAL only: in the global modes the window is beta."""
    if not routes:
        return []
    ops, off = _routes_to_ops(routes)
    r_cat, r_off = _lib._cat(list(reads))
    try:
        md, md_off = _lib.md_batch_by_offset(params, r_cat, r_off, [w[0] for w in windows], [w[1] for w in windows], ops, off)
    except _lib.GnxError as e:
        _raise(e)
    return _lib.md_strings(md, md_off)


def Mapq(scores, second_scores):
    """gnx_mapq_batch: the library's MAPQ (0 .. 60) of placements from their scores and the best score among each one's other
    candidates; None = there is no other candidate."""
    if not len(scores):
        return []
    none = np.iinfo(np.int64).min
    try:
        out = _lib.mapq_batch([int(x) for x in scores], [none if x is None else int(x) for x in second_scores])
    except _lib.GnxError as e:
        _raise(e)
    return [int(x) for x in out]


def _report(params, reads, placed, extra, tags=False):
    """placed[r] = (best, strand, score, window (start, len) or None, route): one SummarizeByOffset call on the reads that have a winner;
    tags: one MDTagsByOffset call on the same reads behind it ("md"), and "mapq" from score and extra[r]["second_score"]"""
    idx = [r for r, p in enumerate(placed) if p[0] >= 0]
    oriented = [dna.ReverseComplement(np.array(reads[r], dtype=np.uint8)) if placed[r][1] else reads[r] for r in idx]  # (it works in place: on a copy)
    sums = SummarizeByOffset(params, oriented, [placed[r][3] for r in idx], [placed[r][4] for r in idx], xcigar=True)
    if tags:
        mds = dict(zip(idx, MDTagsByOffset(params, oriented, [placed[r][3] for r in idx], [placed[r][4] for r in idx])))
        mapq = Mapq([p[2] for p in placed], [e["second_score"] for e in extra])
        extra = [dict(e, md=mds.get(r), mapq=mapq[r]) for r, e in enumerate(extra)]
    at = dict(zip(idx, sums))
    rep = []
    for r, (best, strand, score, win, route) in enumerate(placed):
        d = {"best": best, "strand": strand, "score": score, "window_start": win[0] if win else None, "pos": None, "end": None, "route": route, "xcigar": []}
        if r in at:
            d.update(at[r])
            d["pos"], d["end"] = win[0] + d["alpha_start"], win[0] + d["alpha_end"]
        else:
            d.update({f: 0 for f in _lib.SUMMARY_FIELDS})
        d.update(extra[r])
        rep.append(d)
    return rep


def _local_only(params, name):
    if params.mode != _lib.GNX_AFFINE_GAP_LOCAL:
        raise ValueError("%s: the mode must be GNX_AFFINE_GAP_LOCAL (positions are defined nowhere else)" % name)


def MapReadsReport(params, reads, tags=False, **vote_opts):
    """MapReads (GNX_AFFINE_GAP_LOCAL) plus what is in each placement: the seed and best-of calls run unchanged, then ONE
    SummarizeByOffset call on the winners (strand-1 winners as their reverse complements).  Returns one dict per read: best, strand,
    score, window_start, pos (0-based reference position of the first aligned base = window_start + alpha_start), end, route, xcigar
    and the summary fields; a read without a candidate has best -1, pos None and zero counts.  With tags=True one MDTagsByOffset call
    on the winners follows, and every dict also has md (None for an unplaced read), second_score (the highest score among the read's
    other candidates, None with a single one) and mapq (Mapq of score and second_score)."""
    _local_only(params, "MapReadsReport")
    if not reads:
        return []
    r_cat, r_off = _lib._cat(list(reads))
    try:
        c_off, start, ln, strand, _ = _lib.seed_candidates(r_cat, r_off, **_vote_opts(vote_opts))
        best, scores, _, cand, ops, off = _lib.best_of_by_offset(params, r_cat, r_off, c_off, start, ln, strand, cigar=True)
    except _lib.GnxError as e:
        _raise(e)
    placed = []
    for r in range(len(reads)):
        b = int(best[r])
        c = int(c_off[r]) + b
        placed.append((b, int(strand[c]) if b >= 0 else 0, int(scores[r]), (int(start[c]), int(ln[c])) if b >= 0 else None, _to_route(ops[off[r]:off[r + 1]])))
    if not tags:
        return _report(params, reads, placed, [{} for _ in reads])
    extra = []
    for r in range(len(reads)):
        others = [int(x) for k, x in enumerate(cand[c_off[r]:c_off[r + 1]]) if k != int(best[r])]
        extra.append({"second_score": max(others) if others else None})
    return _report(params, reads, placed, extra, tags=True)


def MapReadPairsReport(params, reads, min_insert, max_insert, unpaired_penalty=0, tags=False, **vote_opts):
    """MapReadPairs plus what is in each placement (see MapReadsReport); every dict also has second_score (None without another
    candidate) and its pair's proper / tlen, and with tags=True md and mapq."""
    _local_only(params, "MapReadPairsReport")
    if len(reads) % 2:
        raise ValueError("MapReadPairsReport: reads come in mate pairs (an even number)")
    if not reads:
        return []
    r_cat, r_off = _lib._cat(list(reads))
    try:
        c_off, start, ln, strand, _ = _lib.seed_candidates(r_cat, r_off, **_vote_opts(vote_opts))
        out = _lib.best_pair_by_offset(params, _lib.pair_opts(min_insert, max_insert, unpaired_penalty), r_cat, r_off, c_off, start, ln, strand, cigar=True)
    except _lib.GnxError as e:
        _raise(e)
    placed, extra = [], []
    for r in range(len(reads)):
        b = int(out["best"][r])
        c = int(c_off[r]) + b
        placed.append((b, int(strand[c]) if b >= 0 else 0, int(out["score"][r]), (int(start[c]), int(ln[c])) if b >= 0 else None,
                       _to_route(out["ops"][out["off"][r]:out["off"][r + 1]])))
        second = int(out["second_score"][r])
        extra.append({"second_score": second if second != np.iinfo(np.int64).min else None, "proper": bool(out["proper"][r // 2]), "tlen": int(out["tlen"][r // 2])})
    return _report(params, reads, placed, extra, tags=tags)


# ---- the pile: per-base counts of placed reads on the resident reference, and the calls they give (gnx_pileup_*) ----
def PileupOpen(start, length):
    """A zeroed pile over [start, start + length) of the resident reference (gnx_pileup_open); an open pile is replaced.  The pile
    belongs to the reference: setting or releasing the reference drops it."""
    try:
        _lib.pileup_open(start, length)
    except _lib.GnxError as e:
        _raise(e)


def PileupClose():
    try:
        _lib.pileup_close()
    except _lib.GnxError as e:
        _raise(e)


def PileupInfo():
    """{"start", "len", "reads_added", "device_bytes"} of the open pile"""
    try:
        return _lib.pileup_info()
    except _lib.GnxError as e:
        _raise(e)


def _phred(q):
    """one read's qualities as raw Phred bytes: a uint8 array as it is, a str / bytes as ASCII + 33"""
    if isinstance(q, (str, bytes)):
        v = np.frombuffer(q.encode("ascii") if isinstance(q, str) else q, dtype=np.uint8)
        if v.size and v.min() < 33:
            raise ValueError("a quality character below '!' (ASCII 33)")
        return v - 33
    return np.asarray(q, dtype=np.uint8)


def PileupAdd(params, reads, windows, strands, routes, use=None, quals=None):
    """Add finished alignments to the open pile (gnx_pileup_add_by_offset, GNX_AFFINE_GAP_LOCAL): windows[k] = (start, len) of the
    resident reference, reads[k] in the orientation it was aligned in (a strand-1 winner: its reverse complement), strands[k] in
    {0, 1} the counter it goes to, routes[k] its CIGAR; use[k] == 0 leaves pair k out.  include/gnx_align.h defines what is counted.
    quals (a pile that tracks qualities, PileupTrackQualities; gnx_pileup_add_by_offset_qual): quals[k] holds one quality per base of
    reads[k], in the same orientation, as a uint8 array of raw Phred values or as a string of ASCII + 33 characters."""
    if not routes:
        return
    ops, off = _routes_to_ops(routes)
    r_cat, r_off = _lib._cat(list(reads))
    try:
        if quals is None:
            _lib.pileup_add_by_offset(params, r_cat, r_off, [w[0] for w in windows], [w[1] for w in windows], strands, ops, off, use=use)
        else:
            quals = [_phred(q) for q in quals]
            if len(quals) != len(reads) or any(len(q) != len(r) for q, r in zip(quals, reads)):
                raise ValueError("PileupAdd: one quality per read base")
            q_cat, _ = _lib._cat(quals)
            _lib.pileup_add_by_offset_qual(params, r_cat, r_off, [w[0] for w in windows], [w[1] for w in windows], strands, ops, off, q_cat, use=use)
    except _lib.GnxError as e:
        _raise(e)


def PileupGet(first=0, count=None):
    """Rows first .. first + count of the open pile (count None: to the end of its region): a structured array with base[2][5]
    ([strand][A C G T N]), del[2] and ins[2] per reference position."""
    try:
        return _lib.pileup_get(first, count)
    except _lib.GnxError as e:
        _raise(e)


def PileupCalls(min_depth, min_alt, frac=(1, 2), both_strands=False):
    """The positions where the reads disagree with the reference, by the library's rule (gnx_pileup_calls): one dict per call, ordered
    by position -- pos, depth, count, count_fwd, kind ("sub" / "del" / "ins"), ref, alt (a base code for a substitution, else None)."""
    try:
        calls = _lib.pileup_calls(min_depth, min_alt, frac[0], frac[1], 1 if both_strands else 0)
    except _lib.GnxError as e:
        _raise(e)
    kinds = ("sub", "del", "ins")
    return [{"pos": int(c["pos"]), "depth": int(c["depth"]), "count": int(c["count"]), "count_fwd": int(c["count_fwd"]), "kind": kinds[int(c["kind"])],
             "ref": int(c["ref"]), "alt": int(c["alt"]) if int(c["kind"]) == 0 else None} for c in calls]


def PileupTrackAlleles(reserve=0):
    """The open pile, still empty, keeps its indel alleles from now on (gnx_pileup_track_alleles): which deletion, which insertion, not
    only how many.  reserve sizes the first log in events (0: a default); the log grows as reads are added."""
    try:
        _lib.pileup_track_alleles(reserve)
    except _lib.GnxError as e:
        _raise(e)


def PileupAlleleInfo():
    """{"tracking", "events", "device_bytes"} of the open pile's allele log"""
    try:
        return _lib.pileup_allele_info()
    except _lib.GnxError as e:
        _raise(e)


_ALLELE_KINDS = (None, "del", "ins", "long_ins")


def _allele_dict(a):
    kind = _ALLELE_KINDS[int(a["kind"])]
    return {"pos": int(a["pos"]), "kind": kind, "length": int(a["length"]), "seq": _lib.unpack_inserted(a["seq"]) if kind == "ins" else None,
            "count": int(a["count"]), "count_fwd": int(a["count_fwd"])}


def PileupAlleles(normalize=False):
    """The distinct indel alleles of a tracking pile with their counts (gnx_pileup_alleles), ordered by position, kind and key: one dict
    each -- pos (a deletion's first deleted base; the base an insertion stands behind), kind ("del" / "ins" / "long_ins"), length, seq
    (the inserted base codes for "ins", else None: a long insertion keeps its length only), count, count_fwd.
    normalize=True (gnx_pileup_alleles_norm): every allele is first moved to its leftmost placement against the reference inside the
    pile's region, so the placements of one deletion along a homopolymer or a tandem repeat are one allele with the summed counts; a
    long insertion stays where it is.  The pile and its log are not changed."""
    try:
        return [_allele_dict(a) for a in _lib.pileup_alleles(normalize=bool(normalize))]
    except _lib.GnxError as e:
        _raise(e)


def PileupIndelCalls(min_depth, min_alt, frac=(1, 2), both_strands=False, normalize=False):
    """The alleles that pass the library's rule (gnx_pileup_indel_calls), in PileupAlleles' order: its dicts plus depth and ref.
    normalize=True (gnx_pileup_indel_calls_norm): the rule is put to the left-normalised alleles, with the depth at their new position."""
    try:
        calls = _lib.pileup_indel_calls(min_depth, min_alt, frac[0], frac[1], 1 if both_strands else 0, normalize=bool(normalize))
    except _lib.GnxError as e:
        _raise(e)
    return [dict(_allele_dict(c), depth=int(c["depth"]), ref=int(c["ref"])) for c in calls]


def PileupTrackQualities(min_baseq=0):
    """The open pile, still empty, sums the base qualities of what it counts from now on (gnx_pileup_track_qualities), and a read base
    whose quality is below min_baseq (0 .. 93) counts nowhere.  Its reads then come through PileupAdd(..., quals=...)."""
    try:
        _lib.pileup_track_qualities(min_baseq)
    except _lib.GnxError as e:
        _raise(e)


def PileupQualInfo():
    """{"tracking", "min_baseq", "device_bytes"} of the open pile's quality planes"""
    try:
        return _lib.pileup_qual_info()
    except _lib.GnxError as e:
        _raise(e)


def PileupGetQual(first=0, count=None):
    """The quality sums of rows first .. first + count of the open quality pile (count None: to the end of its region): an int32 array
    [count][4], the summed Phred qualities of the counted A C G T bases, both strands."""
    try:
        return _lib.pileup_get_qual(first, count)
    except _lib.GnxError as e:
        _raise(e)


def PileupGenotypes(min_depth, min_qual=0, prior_het=3000, prior_hom=3300):
    """The diploid SNP genotypes of a quality pile by the library's rule (gnx_pileup_genotypes), ordered by position: one dict per
    position whose best genotype is not ref / ref -- pos, gt (1 ref / alt, 2 alt / alt), ref, alt (base codes), pl (three values, 0 for
    the called genotype), gq, qual (all in centi-Phred, 1/100 of a Phred unit), depth, ref_count, alt_count, alt_fwd."""
    try:
        recs = _lib.pileup_genotypes(min_depth, min_qual, prior_het, prior_hom)
    except _lib.GnxError as e:
        _raise(e)
    return [{"pos": int(g["pos"]), "gt": int(g["gt"]), "ref": int(g["ref"]), "alt": int(g["alt"]), "pl": [int(v) for v in g["pl"]], "gq": int(g["gq"]), "qual": int(g["qual"]),
             "depth": int(g["depth"]), "ref_count": int(g["ref_count"]), "alt_count": int(g["alt_count"]), "alt_fwd": int(g["alt_fwd"])} for g in recs]


def PileupAddReport(params, reads, report, min_mapq=0, quals=None):
    """Add the placed reads of a MapReadsReport / MapReadPairsReport(tags=True) report whose mapq is at least min_mapq, in ONE call:
    strand-1 reads go in as their reverse complements (as the report's own summaries took them), the window is window_start and the
    alpha bases the route consumes, and `use` leaves out the reads below min_mapq.  quals (a quality pile): one entry per read as
    PileupAdd takes them, in the read's own orientation -- those of a strand-1 read are reversed here.  Returns how many reads it added."""
    idx = [r for r, d in enumerate(report) if d["best"] >= 0]
    if not idx:
        return 0
    oriented = [dna.ReverseComplement(np.array(reads[r], dtype=np.uint8)) if report[r]["strand"] else reads[r] for r in idx]  # (it works in place: on a copy)
    routes = [report[r]["route"] for r in idx]
    windows = [(report[r]["window_start"], sum(c[0] for c in route if c[1] != ColI)) for r, route in zip(idx, routes)]
    use = [1 if report[r]["mapq"] >= min_mapq else 0 for r in idx]
    if quals is not None:
        quals = [_phred(quals[r])[::-1] if report[r]["strand"] else _phred(quals[r]) for r in idx]
    PileupAdd(params, oriented, windows, [report[r]["strand"] for r in idx], routes, use=use, quals=quals)
    return sum(use)


def AffineGapChunk(alpha, beta, scores, gapOpen, gapExtend, chunkSize):
    """align.AffineGapChunk (/root/reference/align/affineGap_highMem.go:227-268)."""
    try:
        sc, ops, off = _lib.affine_gap_chunk_batch(_lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend), chunkSize, [alpha], [beta])
    except _lib.GnxError as e:
        _raise(e)
    return int(sc[0]), _to_route(ops[off[0]:off[1]])


def _groups_to_blocks(groups):
    return [np.stack([np.asarray(f.Seq, dtype=np.uint8) for f in g]) for g in groups]


def multipleAffineGapBatch(groups, pairs, scores, gapOpen, gapExtend, chunkSize=1):
    """multipleAffineGap / multipleAffineGapChunk (affineGap_highMem.go:270-353) for many pairs of fasta groups at once."""
    try:
        sc, ops, off = _lib.multiple_affine_gap_batch(_lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend), chunkSize,
                                                      _groups_to_blocks(groups), pairs)
    except _lib.GnxError as e:
        _raise(e)
    return [(int(sc[k]), _to_route(ops[off[k]:off[k + 1]])) for k in range(len(pairs))]


def mergeMultipleAlignments(alpha, beta, route):
    """align/multiAlign.go:112-153: merge two fasta groups along a cigar (host-side, no DP)."""
    from .fasta import Fasta
    total = sum(c.RunLength for c in route)
    rows = [np.full(total, dna.Gap, dtype=np.uint8) for _ in range(len(alpha) + len(beta))]
    acol = bcol = col = 0
    for c in route:
        n = c.RunLength
        if c.Op in (ColM, ColD):
            for k, f in enumerate(alpha):
                rows[k][col:col + n] = np.asarray(f.Seq, dtype=np.uint8)[acol:acol + n]
        if c.Op in (ColM, ColI):
            for k, f in enumerate(beta):
                rows[len(alpha) + k][col:col + n] = np.asarray(f.Seq, dtype=np.uint8)[bcol:bcol + n]
        if c.Op != ColI:
            acol += n
        if c.Op != ColD:
            bcol += n
        col += n
    return [Fasta(f.Name, rows[k]) for k, f in enumerate(list(alpha) + list(beta))]


def AffineGapChunkScore(alpha, beta, scores, gapOpen, gapExtend, chunkSize):
    """The score AffineGapChunk returns, without its route."""
    try:
        sc = _lib.affine_gap_chunk_score_batch(_lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend), chunkSize, [alpha], [beta])
    except _lib.GnxError as e:
        _raise(e)
    return int(sc[0])


def multipleAffineGapScoreBatch(groups, pairs, scores, gapOpen, gapExtend, chunkSize=1):
    """The scores multipleAffineGapBatch returns for the same arguments, as a list of ints, without the routes."""
    try:
        sc = _lib.multiple_affine_gap_score_batch(_lib.make_params(_lib.GNX_AFFINE_GAP_HIGHMEM, scores, gapOpen, gapExtend), chunkSize,
                                                  _groups_to_blocks(groups), pairs)
    except _lib.GnxError as e:
        _raise(e)
    return [int(x) for x in sc]


def _is_symmetric(scoreMatrix):
    m = [list(row) for row in scoreMatrix]
    return all(m[a][b] == m[b][a] for a in range(len(m)) for b in range(len(m)))


def _all_seq(records, scoreMatrix, gapOpen, gapExtend, chunkSize, batch_fn=None, score_fn=None):
    # multiAlign.go:27-78: progressive alignment, merging the best-scoring pair of groups each round
    # (first strict maximum in x<y order, nearestGroups :27-41).
    # Score first: a round scores the pairs it has no score for in one score_fn call, and only its winner goes through batch_fn for the
    # route.  Scores are remembered under (id of the x group, id of the y group); a merged group gets a fresh id.  groups[y] = groups[-1]
    # moves the last group forward, so later rounds meet pairs with their sides exchanged: score(A, B, S) == score(B, A, S^T), so an
    # exchanged pair reuses its score when the matrix equals its transpose (all four matrices of align.go do).
    # GNX_N1_SCORE_FIRST (read per call): 1 = score first; 0 or unset = every pair with its route, every round, through batch_fn alone.
    # That is the default because it measured faster on cmd/faChunkAlign's workload (8 x 30 kb, chunk 3: 0.072 s against 0.082 s,
    # DESIGN.md 4.17): a call of a few long pairs is bound by the latency of one pair, where the stored-matrix kernel is the quicker one.
    batch_fn = batch_fn or multipleAffineGapBatch
    score_fn = score_fn or multipleAffineGapScoreBatch
    score_first = os.environ.get("GNX_N1_SCORE_FIRST", "0") not in ("0", "")
    symmetric = _is_symmetric(scoreMatrix)
    groups = [[r] for r in records]
    ids = list(range(len(groups)))
    next_id = len(groups)
    known = {}
    while len(groups) > 1:
        pairs = [(x, y) for x in range(len(groups) - 1) for y in range(x + 1, len(groups))]
        if score_first:
            def remembered(x, y):
                s = known.get((ids[x], ids[y]))
                return known.get((ids[y], ids[x])) if s is None and symmetric else s
            todo = [(x, y) for x, y in pairs if remembered(x, y) is None]
            if todo:
                for (x, y), s in zip(todo, score_fn(groups, todo, scoreMatrix, gapOpen, gapExtend, chunkSize)):
                    known[(ids[x], ids[y])] = int(s)
            best, best_score = None, None
            for x, y in pairs:
                score = remembered(x, y)
                if best_score is None or score > best_score:
                    best, best_score = (x, y), score
            x, y = best
            (score, route), = batch_fn(groups, [(x, y)], scoreMatrix, gapOpen, gapExtend, chunkSize)
            if score != best_score:
                raise RuntimeError("progressive alignment: the alignment of groups %d and %d scores %d, their score call gave %d" % (x, y, score, best_score))
        else:
            res = batch_fn(groups, pairs, scoreMatrix, gapOpen, gapExtend, chunkSize)
            best, best_score = None, None
            for (x, y), (score, route) in zip(pairs, res):
                if best_score is None or score > best_score:
                    best, best_score = (x, y, route), score
            x, y, route = best
        groups[x] = mergeMultipleAlignments(groups[x], groups[y], route)
        ids[x] = next_id
        next_id += 1
        groups[y] = groups[-1]
        ids[y] = ids[-1]
        groups = groups[:-1]
        ids = ids[:-1]
        live = set(ids)
        known = {k: v for k, v in known.items() if k[0] in live and k[1] in live}
    return groups[0]


def AllSeqAffine(records, scoreMatrix, gapOpen, gapExtend):
    """align.AllSeqAffine (/root/reference/align/multiAlign.go:59-66)."""
    return _all_seq(records, scoreMatrix, gapOpen, gapExtend, 1)


def AllSeqAffineChunk(records, scoreMatrix, gapOpen, gapExtend, chunkSize):
    """align.AllSeqAffineChunk (/root/reference/align/multiAlign.go:70-78)."""
    return _all_seq(records, scoreMatrix, gapOpen, gapExtend, chunkSize)


class TargetQueryPair:
    """align.TargetQueryPair (affineGap_highMem.go:110-115)."""
    __slots__ = ("Target", "Query", "Score", "Cigar")

    def __init__(self, Target=None, Query=None, Score=0, Cigar=None):
        self.Target, self.Query, self.Score, self.Cigar = Target, Query, Score, Cigar


class _Engine:
    """FIFO batched stand-in for the two channels of GoAffineGapLocalEngine: `send` queues a pair,
    `recv` returns results strictly in input order (the Go engine has one worker goroutine)."""

    def __init__(self, scores, gapOpen, gapExtend, max_batch=1000):
        self._params = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, scores, gapOpen, gapExtend)
        self._pending, self._done, self._max = [], [], max_batch
        self._closed = False

    def send(self, pair):
        if self._closed:
            raise RuntimeError("send on closed channel")
        self._pending.append(pair)
        if len(self._pending) >= self._max:
            self._flush()

    def _flush(self):
        if not self._pending:
            return
        res = AlignBatch(self._params, [p.Target for p in self._pending], [p.Query for p in self._pending])
        for p, (s, c) in zip(self._pending, res):
            p.Score, p.Cigar = s, c
            self._done.append(p)
        self._pending = []

    def recv(self):
        if not self._done:
            self._flush()
        if not self._done:
            if self._closed:
                return None
            raise RuntimeError("recv would block: nothing was sent")
        return self._done.pop(0)

    def close(self):
        self._closed = True

    def __iter__(self):
        while True:
            r = self.recv() if (self._done or self._pending) else None
            if r is None:
                return
            yield r


def GoAffineGapLocalEngine(scores, gapOpen, gapExtend):
    """Returns (inputs, outputs); both are the same FIFO engine object (inputs.send / outputs.recv)."""
    e = _Engine(scores, gapOpen, gapExtend)
    return e, e


def _col_rune(op):
    if op == ColM:
        return "M"
    if op == ColI:
        return "I"
    if op == ColD:
        return "D"
    raise ValueError("Error: unexpected value when converting colType to rune %d" % op)


def PrintCigar(operations):
    return "".join("%d%s" % (c.RunLength, _col_rune(c.Op)) for c in operations)


def FormatCigar(operations):
    """Go's fmt %v of a []Cigar, e.g. `[{2 0} {1 1}]` (cmd/globalAlignmentAnchor.go:23-27)."""
    return "[" + " ".join("{%d %d}" % (c.RunLength, c.Op) for c in operations) + "]"


def View(alpha, beta, operations):
    one, two = [], []
    i = j = 0
    a = dna.BasesToString(np.asarray(alpha, dtype=np.uint8))
    b = dna.BasesToString(np.asarray(beta, dtype=np.uint8))
    for c in operations:
        n = c.RunLength
        if c.Op == ColM:
            one.append(a[i:i + n]); two.append(b[j:j + n]); i += n; j += n
        elif c.Op == ColI:
            one.append("-" * n); two.append(b[j:j + n]); j += n
        elif c.Op == ColD:
            one.append(a[i:i + n]); two.append("-" * n); i += n
    return "".join(one) + "\n" + "".join(two) + "\n"
