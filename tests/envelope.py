"""The numeric admission rules of the kernel routes, restated, and the cases that sit ON them (tests/test_envelope_cpu.py,
tests/test_envelope_gpu.py; DESIGN.md "Numeric envelope").

Every route of run_device, run_score_sweep and the chunk driver is admitted by a rule on the score table, the penalties and the
shape; the kernel behind it then leans on the rule (padding rows of -32768, sentinels of -2^30, profiles packed two to a dword).
Here each rule is one pure predicate written from its meaning -- no GPU, no ctypes anywhere in this module (the oracle's results
for a case come from tests/envelope_oracle.py) -- and one builder that returns parameter sets
whose controlling expression is the LAST value the rule admits (upper and lower end) and the FIRST it refuses (one integer step on
one score, one penalty, or one base of length beyond).  The extreme entry is on a cell the inputs use: the maximum on A/A, the
minimum on A/C and on N/G; the table is asymmetric (tests/asym.py says why).

A case is a Case tuple; its first six fields are (label, mode, scores, gap_open, gap_extend, admitted)."""
import collections
import functools

import numpy as np

import common  # (numpy only: the mutation model the other suites' batches use)

AFFINE_MODES = (0, 2, 3)  # AffineGap, AffineGap_highMem, AffineGapLocal
CONST_MODES = (1, 4)      # ConstGap, ConstGap_highMem
GLOBAL_MODES = (0, 1, 2, 4)
LOCAL = 3
A, C, G, T, N = range(5)
HI_CELL = (A, A)            # where the largest entry of a table is
LO_CELLS = ((A, C), (N, G))  # where the smallest is: one off-diagonal cell, one cell of the N row

# the kernels' geometry the rules are written in (gnx_common.hip.h, affine_long*.hip.h, const_long*.hip.h, score_sweep.hip.h)
H16, G16, H64, G64 = 160, 16, 640, 64
CKA, CKC, CKC64 = 128, 448, 224
RB_PUB = 64
SS_ROWS = 64 * 160  # SS_MAX_LEVELS row blocks of 160 rows

Case = collections.namedtuple("Case", "label mode scores gap_open gap_extend admitted rule total chunk undo extreme")
# total: n + m + 2 of the pairs, for the rules that bound a shape (None: the shape is free);  chunk: chunkSize of the N1 calls;
# undo: the one step that takes a first-refused set back to the last admitted one;  extreme: "hi" / "lo" / None -- which extreme
# entry of the table the set is about


def affine(mode):
    return mode in AFFINE_MODES


def ge_of(mode, gap_extend):
    """what the library reads: the constant-gap functions have no gapExtend"""
    return gap_extend if affine(mode) else 0


def flat(scores):
    return [int(v) for row in scores for v in row]


# ---- the rules --------------------------------------------------------------------------------------------------------------------
def max_pen(mode, scores, gap_open, gap_extend):
    """max_abs_pen(prm, affine) of gnx_align.hip: the largest step a key can take"""
    v = [abs(s) for s in flat(scores)] + [abs(gap_open)]
    if affine(mode):
        v += [abs(gap_extend), abs(gap_open + gap_extend)]
    return max(v)


def k27(mode, scores, gap_open, gap_extend, n, m):
    """K27 -- the validation loop of run_device (first_oor): static int32 keys hold 4 * score of every cell of the pair"""
    return (n + m + 2) * max(max_pen(mode, scores, gap_open, gap_extend), 1) < (1 << 27)


def k27_last_total(mode, scores, gap_open, gap_extend):
    """the largest n + m + 2 K27 admits"""
    return ((1 << 27) - 1) // max(max_pen(mode, scores, gap_open, gap_extend), 1)


def p26(mode, scores, gap_open, gap_extend):
    """P26 -- check_params: what 4 * x still fits int32 for with room for one addition; beyond it GNX_ERANGE"""
    lim = 1 << 26
    return all(abs(s) <= lim for s in flat(scores)) and abs(gap_open) <= lim and (not affine(mode) or abs(gap_extend) <= lim)


def fp16(mode, scores, gap_open, gap_extend):
    """FP16 -- the fast-path block of run_device: fp_sweep_kernel's int16 profile of 4 * (s - 2e), padding rows that need
    4 * |gapOpen| well inside int16, and for the transposed (AffineGapLocal) form a gapExtend that is a real penalty"""
    if not affine(mode) or not (-8000 < gap_open <= 0):
        return False
    if mode == LOCAL and not (-8000 < gap_extend < 0):
        return False
    return all(-32000 <= 4 * (s - 2 * gap_extend) <= 32767 for s in flat(scores))


def sn16(mode, scores, gap_open, gap_extend):
    """SN16 -- snap_profile_fits_int16: the snapshot path's rebased profile 4 * (s - 2g) + 1, g = gapExtend (affine) or the gap"""
    g = gap_extend if affine(mode) else gap_open
    return all(-32768 <= 4 * (s - 2 * g) + 1 <= 32767 for s in flat(scores))


def gp16(mode, scores, gap_open, gap_extend, plain=False):
    """GP16 -- the plan section of run_device (`p16`, read only under GNX_FORCE_P16 and only by fill_affine_kernel's launch: the
    constant-gap fill takes its profile width from CP16 alone).  The kernel's rebased tables (h-form: gapOpen <= 0 and no
    GNX_NO_HFORM) store 4 * (s - 2e); its plain ones store 4 * s, which then has to fit as well (plain: GNX_NO_HFORM is set)"""
    e = gap_extend if affine(mode) else 0
    hform = affine(mode) and gap_open <= 0 and not plain
    return all(-32768 <= 4 * (s - 2 * e) <= 32767 and (hform or -32768 <= 4 * s <= 32767) for s in flat(scores))


def gp16_is_plain(case):
    """the sets that are run with GNX_NO_HFORM (the others with gapOpen > 0 have the plain tables by themselves)"""
    return " plain" in case.label


def cp16(mode, scores, gap_open, gap_extend):
    """CP16 -- the constant-gap launch of run_device (`cp16`): piped fill_const_kernel's profile 4 * (s - 2 gap) + 1"""
    return not affine(mode) and all(-32768 <= 4 * (s - 2 * gap_open) + 1 <= 32767 for s in flat(scores))


def ss_params(mode, scores, gap_open, gap_extend):
    """SS, the part on the parameters -- run_score_sweep (n1_sweep_fits has the same on the scaled parameters): gapOpen and the
    profile s - 2 * reb inside int16 with room to spare"""
    if not (-16000 <= gap_open <= 0):
        return False
    if mode == LOCAL and not (-8000 <= gap_extend <= 0):
        return False
    reb = gap_extend if affine(mode) else gap_open
    return all(-16000 <= s - 2 * reb <= 16000 for s in flat(scores))


def ss_keys(mode, scores, gap_open, gap_extend, n, m):
    """SS, the part on the shape -- run_score_sweep: the rebased keys inside int32, the side held in lanes at most 64 row blocks"""
    rows = m if mode == LOCAL else min(n, m)  # (AffineGapLocal: the query, whatever the lengths)
    return n >= 1 and m >= 1 and rows <= SS_ROWS and (n + m + 2) * 2 * max(max_pen(mode, scores, gap_open, gap_extend), 1) < (1 << 30)


def ss(mode, scores, gap_open, gap_extend, n, m):
    return ss_params(mode, scores, gap_open, gap_extend) and ss_keys(mode, scores, gap_open, gap_extend, n, m)


def ss_last_total(mode, scores, gap_open, gap_extend):
    return ((1 << 29) - 1) // max(max_pen(mode, scores, gap_open, gap_extend), 1)


def n1_s16(scores, gap_open, gap_extend, chunk):
    """N1 -- run_host_scored (`s16`): the explicit score matrix of the chunk / multiple-alignment calls as int16.  An entry is
    4 * (a sum of `chunk` scores); the h-form and the sweep (gapOpen <= 0) add the -8 * gapExtend * chunk of the diagonal move"""
    smax = max(abs(s) for s in flat(scores))
    bias = abs(8 * gap_extend * chunk) if gap_open <= 0 else 0
    return 4 * chunk * smax + bias <= 32767


def step4(mode, scores, gap_open, gap_extend):
    """the snapshot block of run_device: how far two neighbouring keys of a strip on a moving base can be apart (x 4)"""
    mp = max([abs(s) for s in flat(scores)] + [abs(gap_open)])
    return 4 * (mp + 2 * abs(gap_open) + (2 * abs(gap_extend) if affine(mode) else 0))


def spr_moving(mode, scores, gap_open, gap_extend):
    """SPR, moving bases at all (`spread_ok`): a 16-lane strip's band, the row above and the widest snapshot spacing"""
    return (H16 + G16 + max(CKC, CKA) + 64) * step4(mode, scores, gap_open, gap_extend) < (1 << 28)


def spr_w64_ck(mode, scores, gap_open, gap_extend):
    """SPR, the snapshot spacing of the 64-lane affine sweep (`t_w64_ck`): the widest of 512, 256 the spread admits, else 128;
    the constant-gap form has one spacing (CKC64)"""
    if not affine(mode):
        return CKC64
    for ck in (512, 256):
        if (H64 + G64 + ck + 64) * step4(mode, scores, gap_open, gap_extend) < (1 << 28):
            return ck
    return CKA


def spr_w64(mode, scores, gap_open, gap_extend):
    """SPR, the 64-lane kernels at all (`w64`): the code bounds both forms with max(CKC64, the chosen spacing) -- at the narrowest
    affine spacing, 128, that is the constant-gap form's 224, not 128"""
    ck = max(CKC64, spr_w64_ck(mode, scores, gap_open, gap_extend))
    return (H64 + G64 + ck + 64) * step4(mode, scores, gap_open, gap_extend) < (1 << 28)


def spr_mega_ck(mode, scores, gap_open, gap_extend, rw=10):
    """SPR, the snapshot spacing of the affine 64-lane sweep in row panels (`ck_mega`, run_device_mega): the widest power of two from
    2 048 down to 128 the spread admits at `rw` rows per lane, else the spacing of the unpanelled sweep"""
    for ck in (2048, 1024, 512, 256, 128):
        if (G64 * rw + G64 + ck + 64) * step4(mode, scores, gap_open, gap_extend) < (1 << 28):
            return ck
    return spr_w64_ck(mode, scores, gap_open, gap_extend)


RULES = {"K27": k27, "P26": p26, "FP16": fp16, "SN16": sn16, "GP16": gp16, "CP16": cp16, "SS": ss, "N1": n1_s16,
         "SPR": spr_moving}


def admitted(case, n=None, m=None):
    """the case's own rule on the case (for the rules on a shape: on a pair with n + m + 2 = case.total)"""
    c = case
    ge = ge_of(c.mode, c.gap_extend)
    if c.rule in ("K27", "SS"):
        if n is None:
            total = c.total if c.total is not None else 200
            n = max(1, min((total - 2) // 2, SS_ROWS))
            m = total - 2 - n
        return RULES[c.rule](c.mode, c.scores, c.gap_open, ge, n, m)
    if c.rule == "N1":
        return n1_s16(c.scores, c.gap_open, ge, c.chunk)
    if c.rule.startswith("SPR"):
        return {"SPR": spr_moving, "SPR64": spr_w64, "SPR512": lambda *a: spr_w64_ck(*a) >= 512, "SPR256": lambda *a: spr_w64_ck(*a) >= 256,
                "SPRM2048": lambda *a: spr_mega_ck(*a) >= 2048, "SPRM1024": lambda *a: spr_mega_ck(*a) >= 1024}[c.rule](c.mode, c.scores, c.gap_open, ge)
    if c.rule == "GP16":
        return gp16(c.mode, c.scores, c.gap_open, ge, plain=gp16_is_plain(c))
    return RULES[c.rule](c.mode, c.scores, c.gap_open, ge)


# ---- tables and steps -------------------------------------------------------------------------------------------------------------
def table(hi, lo):
    """an asymmetric 5 x 5 table inside [lo, hi]: hi on A/A, lo on A/C and N/G, the other diagonal cells in the upper part, the
    other cells in the lower part, table[a][b] != table[b][a] wherever the span leaves room"""
    span = hi - lo
    assert span >= 0
    t = [[(hi - (span * a) // 16) if (a == b and a < 4) else (lo + (span * ((3 * a + 7 * b) % 23 + 1)) // 64) for b in range(5)] for a in range(5)]
    t[A][A] = hi
    for a, b in LO_CELLS:
        t[a][b] = lo
    return t


def stepped(case, what, label=None, admitted_=None, undo=None):
    """the case moved by one step: what = ("score", a, b, d) | ("gap_open", d) | ("gap_extend", d) | ("total", d)"""
    sc = [list(r) for r in case.scores]
    go, ge, total = case.gap_open, case.gap_extend, case.total
    if what[0] == "score":
        sc[what[1]][what[2]] += what[3]
    elif what[0] == "gap_open":
        go += what[1]
    elif what[0] == "gap_extend":
        ge += what[1]
    elif what[0] == "total":
        total += what[1]
    else:
        raise ValueError(what)
    return case._replace(label=label or case.label, scores=sc, gap_open=go, gap_extend=ge, total=total,
                         admitted=case.admitted if admitted_ is None else admitted_, undo=undo)


def _inverse(what):
    return what[:-1] + (-what[-1],)


def _refuse(case, what, label):
    return stepped(case, what, label=label, admitted_=False, undo=_inverse(what))


def _case(rule, label, mode, scores, go, ge, extreme=None, total=None, chunk=None):
    return Case(label, mode, scores, go, ge_of(mode, ge), True, rule, total, chunk, None, extreme)


def _hi_lo_steps(case, tag):
    """the first refused sets beyond a table's two ends: + 1 on the maximum (A/A), - 1 on the minimum (A/C, and N/G alone)"""
    out = []
    if case.extreme in ("hi", "both"):
        out.append(_refuse(case, ("score", A, A, 1), tag + " max + 1"))
    if case.extreme in ("lo", "both"):
        out.append(_refuse(case, ("score", A, C, -1), tag + " min - 1 (A/C)"))
        out.append(_refuse(case, ("score", N, G, -1), tag + " min - 1 (N/G)"))
    return out


# ---- the builders -----------------------------------------------------------------------------------------------------------------
def k27_cases():
    """per mode a positive family (|score| = 2^20 on A/A: an all-match pair ends near + 2^27 / 2), an all-negative one (- 2^20 on
    A/C, gaps as dear: an all-mismatch pair ends near - 2^27 / 2) and, for the 64-lane kernels, which SPR refuses such scores, one
    at the largest score SPR admits them with; each at the last total admitted and the first refused (and at 2^27 // maxpen - 1 /
    + 1 where these are other totals); then the families that FP16 admits too, for the fast path: the rule's ends at totals of
    1 242 .. 16 170, whose keys come from long gap runs"""
    out = []
    big = 1 << 20
    for mode in range(5):
        go = -600 if affine(mode) else -430
        fams = [("pos", table(big, -(big >> 1)), go, -150), ("neg", table(-3, -big), 0 if affine(mode) else -big, -big)]
        if mode != LOCAL:  # the largest score under which SPR still admits the 64-lane kernels: pairs of 1 013 bases a side
            s64 = _spr_last_step4(H64 + G64 + CKC64 + 64) // 4 - 2 * abs(go) - (300 if affine(mode) else 0)
            fams.append(("w64", table(s64, -(s64 // 2)), go, -150))
        for tag, sc, go, ge in fams:
            base = _case("K27", "", mode, sc, go, ge)
            last = k27_last_total(mode, sc, go, base.gap_extend)
            mp = max_pen(mode, sc, go, base.gap_extend)
            adm = base._replace(label="K27 m%d %s last" % (mode, tag), total=last)
            out.append(adm)
            if (1 << 27) // mp - 1 != last:
                out.append(base._replace(label="K27 m%d %s 2^27//maxpen-1" % (mode, tag), total=(1 << 27) // mp - 1))
            out.append(_refuse(adm, ("total", 1), "K27 m%d %s first refused" % (mode, tag)))
            if (1 << 27) // mp + 1 != last + 1:
                out.append(base._replace(label="K27 m%d %s 2^27//maxpen+1" % (mode, tag), total=(1 << 27) // mp + 1, admitted=False))
    for mode, tag, go, ge in ((0, "fp gaps", -7999, -50000), (0, "fp", -7999, -150), (LOCAL, "fp", -7999, -7999)):
        sc = table(8191 + 2 * ge, -8000 + 2 * ge)
        assert fp16(mode, sc, go, ge)
        base = _case("K27", "", mode, sc, go, ge)
        adm = base._replace(label="K27 m%d %s last" % (mode, tag), total=k27_last_total(mode, sc, go, ge))
        out += [adm, _refuse(adm, ("total", 1), "K27 m%d %s first refused" % (mode, tag))]
    return out


def k27_is_fast_path_family(case):
    return " fp" in case.label


def p26_cases():
    lim = 1 << 26
    out = []
    for mode in range(5):
        adm = _case("P26", "P26 m%d last" % mode, mode, table(lim, -lim), -lim, -lim, extreme="both")
        out.append(adm)
        out += _hi_lo_steps(adm, "P26 m%d" % mode)
        out.append(_refuse(adm, ("gap_open", -1), "P26 m%d gapOpen - 1" % mode))
        if affine(mode):
            out.append(_refuse(adm, ("gap_extend", -1), "P26 m%d gapExtend - 1" % mode))
        pos = _case("P26", "P26 m%d last, gaps > 0" % mode, mode, table(lim, -lim), lim, lim, extreme="both")
        out += [pos, _refuse(pos, ("gap_open", 1), "P26 m%d gapOpen + 1" % mode)]
    return out


def fp16_cases():
    """4 * (s - 2e) = 32 764 (the largest multiple of 4 inside int16) and - 32 000, gapOpen = - 7 999 and 0, the transposed form's
    gapExtend = - 7 999 and - 1; one step beyond each"""
    out = []
    for mode, ge in ((0, -150), (0, -7999), (2, -150), (LOCAL, -150), (LOCAL, -7999), (LOCAL, -1)):
        tag = "FP16 m%d e%d" % (mode, ge)
        adm = _case("FP16", tag + " last", mode, table(8191 + 2 * ge, -8000 + 2 * ge), -7999, ge, extreme="both")
        out.append(adm)
        out += _hi_lo_steps(adm, tag)
        out.append(_refuse(adm, ("gap_open", -1), tag + " gapOpen - 1"))
        if mode == LOCAL and ge in (-7999, -1):  # (gapExtend moves the profile too: the step is taken on a table with room for it)
            slack = _case("FP16", tag + " last, table with room", mode, table(8100 + 2 * ge, -7900 + 2 * ge), -7999, ge)
            d = -1 if ge == -7999 else 1
            out += [slack, _refuse(slack, ("gap_extend", d), tag + " gapExtend %+d" % d)]
    for mode in (0, LOCAL):
        # (no mismatch dearer than two gap bases here, and the test runs it on sides of about one length: with gaps free to open, CIGARs
        # outgrow the runs the fast path stages, and a batch of them goes back to the general path)
        zero = _case("FP16", "FP16 m%d gapOpen 0 last" % mode, mode, table(8191 - 300, -200), 0, -150, extreme="hi")
        out += [zero, _refuse(zero, ("gap_open", 1), "FP16 m%d gapOpen + 1" % mode)]
    return out


def _profile_cases(rule, modes, hi_expr, lo_expr, gaps):
    """the int16 profile rules: entry(s) = 4 * (s - 2g) + c; a family with the maximum on A/A at the largest admitted s, and one with
    the minimum at the smallest (whose gaps are dear enough for a mismatch to be worth taking, where the arithmetic allows it)"""
    out = []
    for mode in modes:
        for end, (go, ge) in zip(("hi", "lo"), gaps(mode)):
            g = (ge if affine(mode) else go) if rule != "GP16" else (ge if affine(mode) else 0)
            hi, lo = hi_expr + 2 * g, lo_expr + 2 * g
            sc = table(hi, hi - 9000) if end == "hi" else table(lo + 16000, lo)  # (the lower end under a diagonal that is worth aligning)
            adm = _case(rule, "%s m%d %s last" % (rule, mode, end), mode, sc, go, ge, extreme=end)
            out.append(adm)
            out += _hi_lo_steps(adm, "%s m%d" % (rule, mode))
    return out


def sn16_cases():
    """4 * (s - 2g) + 1 = 32 765 and - 32 767"""
    return _profile_cases("SN16", GLOBAL_MODES, 8191, -8192, lambda mode: ((-600, -150), (-6000, -150)) if affine(mode) else ((-430, 0), (-430, 0)))


def gp16_cases():
    """4 * (s - 2e) = 32 764 and - 32 768, for fill_affine_kernel<.., P16> (global and local) with the rebased tables; with the
    plain ones (GNX_NO_HFORM, or gapOpen > 0) 4 * s = - 32 768, and 4 * s = 32 764 under a gapExtend > 0"""
    out = _profile_cases("GP16", AFFINE_MODES, 8191, -8192, lambda mode: ((-600, -150), (-6000, -150)))
    for mode in AFFINE_MODES:
        for tag, go, ge in (("plain", -6000, -150), ("gapOpen > 0", 25, -150)):
            adm = _case("GP16", "GP16 m%d %s lo last" % (mode, tag), mode, table(-8192 + 16000, -8192), go, ge, extreme="lo")
            out.append(adm)
            out += _hi_lo_steps(adm, "GP16 m%d %s" % (mode, tag))
        adm = _case("GP16", "GP16 m%d plain, gapExtend > 0, hi last" % mode, mode, table(8191, 8191 - 9000), -6000, 40, extreme="hi")
        out.append(adm)
        out += _hi_lo_steps(adm, "GP16 m%d plain, gapExtend > 0," % mode)
    return out


def cp16_cases():
    """4 * (s - 2 gap) + 1 = 32 765 and - 32 767, for the piped fill_const_kernel<.., P16>"""
    return _profile_cases("CP16", CONST_MODES, 8191, -8192, lambda mode: ((-430, 0), (-430, 0)))


def ss_cases():
    """the score sweeps: s - 2 * reb = + 16 000 / - 16 000, gapOpen = - 16 000 / 0, the local form's gapExtend = - 8 000 / 0, and the
    key range (n + m + 2) * 2 * maxpen < 2^30 at tables whose gap runs carry a pair to - 2^29 / 2"""
    out = []
    for mode in range(5):
        reb_of = (lambda go, ge: ge) if affine(mode) else (lambda go, ge: go)
        tag = "SS m%d" % mode
        for end, (go, ge) in (("hi", (-600, -150) if affine(mode) else (-430, 0)), ("lo", (-16000, -150) if affine(mode) else (-16000, 0))):
            reb = reb_of(go, ge)
            sc = table(16000 + 2 * reb, 16000 + 2 * reb - 9000) if end == "hi" else table(-16000 + 2 * reb + 30000, -16000 + 2 * reb)
            adm = _case("SS", "%s %s last" % (tag, end), mode, sc, go, ge, extreme=end)
            out.append(adm)
            out += _hi_lo_steps(adm, tag)
            if end == "lo":
                out.append(_refuse(adm, ("gap_open", -1), tag + " gapOpen - 1"))
        zgo = _case("SS", tag + " gapOpen 0 last", mode, table(300, -5000), 0, -150)
        out += [zgo, _refuse(zgo, ("gap_open", 1), tag + " gapOpen + 1")]
        if mode == LOCAL:
            e_lo = _case("SS", tag + " gapExtend -8000 last", mode, table(0, -32000), -16000, -8000, extreme="both")
            e_hi = _case("SS", tag + " gapExtend 0 last", mode, table(16000, -16000), -600, 0, extreme="both")
            out += [e_lo, e_hi]
            # (gapExtend moves the profile too: the steps are taken on tables with room for it)
            s_lo = _case("SS", tag + " gapExtend -8000 last, table with room", mode, table(-100, -31900), -16000, -8000)
            s_hi = _case("SS", tag + " gapExtend 0 last, table with room", mode, table(15900, -15900), -600, 0)
            out += [s_lo, _refuse(s_lo, ("gap_extend", -1), tag + " gapExtend - 1"), s_hi, _refuse(s_hi, ("gap_extend", 1), tag + " gapExtend + 1")]
        # the key range: every entry and penalty at its own end too, so that maxpen is as large as the parameters allow
        if affine(mode):
            sc, go, ge = table(0, -32000), -16000, -8000
        else:
            sc, go, ge = table(-16000, -48000), -16000, 0
        base = _case("SS", "", mode, sc, go, ge)
        last = ss_last_total(mode, sc, go, base.gap_extend)
        adm = base._replace(label=tag + " keys last", total=last)
        out += [adm, _refuse(adm, ("total", 1), tag + " keys first refused")]
    return out


def ss_is_key_family(case):
    return " keys " in case.label


def n1_cases():
    """4 * chunk * max|s| + 8 * |gapExtend| * chunk = the largest value <= 32 767, for chunkSize 1 and 3, the maximum on A/A (a dear
    match) and the minimum on A/C (a dear mismatch, gaps dearer still)"""
    out = []
    for chunk in (1, 3):
        ge = -30
        smax = (32767 - 8 * abs(ge) * chunk) // (4 * chunk)
        for end, sc, go in (("hi", table(smax, -smax // 2), -400), ("lo", table(smax // 2, -smax), -6000)):
            adm = _case("N1", "N1 chunk %d %s last" % (chunk, end), 2, sc, go, ge, extreme=end, chunk=chunk)
            out.append(adm)
            out += _hi_lo_steps(adm, "N1 chunk %d" % chunk)
    return out


def _spr_last_step4(width):
    """the largest multiple of 4 with width * step4 < 2^28"""
    return (((1 << 28) - 1) // width) // 4 * 4


SPR_WIDTHS = (("SPRM2048", H64 + G64 + 2048 + 64), ("SPRM1024", H64 + G64 + 1024 + 64), ("SPR512", H64 + G64 + 512 + 64), ("SPR256", H64 + G64 + 256 + 64), ("SPR64", H64 + G64 + CKC64 + 64), ("SPR", H16 + G16 + CKC + 64))


def spr_cases():
    """step4 on each side of each threshold of the moving-base spread, by the size of the score on A/A (the affine forms: six
    thresholds -- spacing 2 048 and 1 024 of row panels at 10 rows per lane, spacing 512 and 256, the 64-lane kernels at all, moving
    bases at all; the constant-gap forms: the last two)"""
    out = []
    for mode in GLOBAL_MODES:
        go, ge = (-600, -150) if affine(mode) else (-430, 0)
        for rule, width in SPR_WIDTHS:
            if not affine(mode) and rule in ("SPRM2048", "SPRM1024", "SPR512", "SPR256"):
                continue
            s = _spr_last_step4(width) // 4 - 2 * abs(go) - (2 * abs(ge) if affine(mode) else 0)
            adm = _case(rule, "%s m%d last" % (rule, mode), mode, table(s, -(s // 3)), go, ge, extreme="hi")
            out += [adm, _refuse(adm, ("score", A, A, 1), "%s m%d first refused" % (rule, mode))]
    return out


def sign_cases():
    """gapOpen = 0 and > 0, gapExtend = 0 and > 0, an all-positive and an all-zero table, at ordinary magnitudes and at 2^20: an
    error code is a valid answer, a wrong alignment is not"""
    out = []
    for mag, tag in ((1, "ordinary"), (1 << 13, "2^20")):
        tables = (("mixed", table(91 * mag, -128 * mag)), ("positive", table(128 * mag, 3 * mag)), ("zero", [[0] * 5 for _ in range(5)]))
        for tname, sc in tables:
            for go, ge in ((0, -30 * mag), (25 * mag, -30 * mag), (-40 * mag, 0), (-40 * mag, 7 * mag), (0, 0), (13 * mag, 5 * mag)):
                for mode in range(5):
                    if not affine(mode) and ge not in (0, -30 * mag):
                        continue  # (the constant-gap functions read gapOpen alone: one set per value of it)
                    out.append(_case("SIGN", "SIGN %s %s m%d (%d, %d)" % (tag, tname, mode, go, ge), mode, sc, go, ge))
    return out


BUILDERS = {"K27": k27_cases, "P26": p26_cases, "FP16": fp16_cases, "SN16": sn16_cases, "GP16": gp16_cases, "CP16": cp16_cases,
            "SS": ss_cases, "N1": n1_cases, "SPR": spr_cases}


@functools.lru_cache(maxsize=None)
def cases(rule):
    return tuple(BUILDERS[rule]())


def by_label(rule, label):
    return [c for c in cases(rule) if c.label == label][0]


# ---- the sequences ----------------------------------------------------------------------------------------------------------------
def split_total(total, rows=None, fracs=(0.5, 0.5, 0.32, 0.16, 0.5, 0.5, 0.01, 0.99, 0.8, 0.25)):
    """shapes (n, m) with n + m + 2 = total: n from `rows`, or the given fractions of n + m"""
    if rows is None:
        rows = [max(1, min(total - 3, int(round(f * (total - 2))))) for f in fracs]
    return [(n, total - 2 - n) if n > 0 else (total - 2 + n, -n) for n in rows]


def pairs(seed, shapes, swap=False):
    """the small batch every parameter set gets, one pair per shape (n, m), in this order: an all-match pair (A against A: the
    maximum), an all-mismatch pair on the minimum cell (A against C), a pair with nothing in common (G against T; n != m forces
    gaps), a read inside a longer window (long leading and trailing gaps), a pair with runs of N (and N against G: the minimum of
    the N row), a sequence against itself with every ninth base an A on one side and a C on the other (isolated mismatches on the
    minimum cell, which an alignment keeps wherever the two gap opens around them would cost more), ragged random pairs for the rest.
    swap: every shape is taken as (m, n) -- AffineGapLocal, whose alpha is the target: the longer side, the window"""
    rng = np.random.default_rng(seed)
    alphas, betas = [], []
    for k, (n, m) in enumerate(shapes):
        if swap:
            n, m = m, n
        if k == 0:
            a, b = np.full(n, A, np.uint8), np.full(m, A, np.uint8)
        elif k == 1:
            a, b = np.full(n, A, np.uint8), np.full(m, C, np.uint8)
        elif k == 2:
            a, b = np.full(n, G, np.uint8), np.full(m, T, np.uint8)
        elif k == 3:
            short, long_ = min(n, m), max(n, m)
            win = rng.integers(0, 4, size=long_).astype(np.uint8)
            off = int(rng.integers(0, long_ - short + 1))
            read = win[off:off + short].copy()
            read[rng.random(short) < 0.03] = A
            a, b = (read, win) if n <= m else (win, read)
        elif k == 4:
            a = rng.integers(0, 4, size=n).astype(np.uint8)
            b = np.resize(a, m).astype(np.uint8)
            b[rng.random(m) < 0.1] = G
            for x, ln in ((a, n), (b, m)):
                p = int(rng.integers(0, max(1, ln - ln // 5)))
                x[p:p + max(1, ln // 5)] = N
            at = np.arange(0, min(n, m), max(2, min(n, m) // 7))
            a[at] = N
            b[at] = G
        elif k == 5:
            a = rng.integers(0, 4, size=n).astype(np.uint8)
            b = np.resize(a, m).astype(np.uint8)
            at = np.arange(4, min(n, m), 9)
            a[at] = A
            b[at] = C
        else:
            a = rng.integers(0, 5, size=n).astype(np.uint8)
            b = common.mutate(rng, a, sub=0.1, indel=0.05, geo=0.4, alphabet=5)
            b = np.concatenate([b, rng.integers(0, 5, size=m).astype(np.uint8)])[:m]
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        assert a.shape[0] == n and b.shape[0] == m, (k, n, m, a.shape, b.shape)
        alphas.append(a)
        betas.append(b)
    return alphas, betas


# named shape lists: the smallest the route under test accepts
SHAPES = {
    "tiny": [(62, 62), (61, 61), (40, 77), (20, 100), (63, 60), (50, 52), (1, 90), (90, 1), (100, 25), (31, 94)],
    # the fast path: reads (rows) of one 160-row block / of two and three, windows of 128 .. 2049 columns
    "fp1": [(160, 160), (150, 150), (97, 300), (150, 1100), (160, 700), (140, 150), (1, 200), (33, 128), (159, 2049), (120, 129), (140, 257)],
    "fp23": [(161, 161), (320, 320), (300, 480), (200, 1100), (480, 700), (300, 310), (161, 300), (321, 2049), (479, 500), (400, 129)],
    # ... for gapOpen = 0, where a window longer than its read costs the same in one gap run or in fifty: sides of about one length
    "fp1 level": [(160, 160), (150, 150), (97, 100), (150, 155), (160, 158), (140, 141), (1, 3), (33, 36), (159, 161), (120, 119)],
    "fp23 level": [(161, 161), (320, 320), (300, 305), (200, 204), (480, 478), (300, 301), (161, 165), (321, 325), (479, 480)],
    # the general path: one strip, several strips walked by one wave (m < 8 * RB_PUB), piped strips (more than 160 rows, m >= 512)
    "strip": [(100, 100), (160, 160), (60, 111), (50, 300), (150, 170), (120, 125), (1, 40), (160, 33), (77, 400)],
    "multi": [(300, 300), (200, 200), (170, 333), (180, 500), (400, 350), (250, 255), (161, 40), (330, 100), (500, 511)],
    "piped": [(300, 512), (512, 512), (170, 700), (200, 1100), (400, 600), (512, 520), (161, 512), (330, 1024), (500, 513)],
    # the snapshot path: several 160-row strips; the 64-lane farm: at least 2 * 640 rows; row panels of three strips
    "snap": [(300, 300), (480, 480), (170, 700), (200, 1100), (700, 600), (320, 330), (161, 512), (650, 900), (500, 513)],
    "farm": [(1280, 1280), (1300, 1300), (1290, 700), (1281, 1500), (1400, 900), (1300, 1310)],
    "panels": [(1000, 1000), (700, 700), (500, 900), (300, 1300), (1100, 600), (700, 705), (961, 512)],
    # the score sweeps: the shorter side in lanes, one to three levels, both sides the shorter one
    "sweep": [(160, 160), (161, 161), (100, 400), (40, 600), (330, 300), (170, 175), (1, 50), (50, 1), (481, 500), (400, 161)],
}
FIRST_SHAPES = {"FP16": "fp1", "SN16": "snap", "GP16": "strip", "CP16": "piped", "SS": "sweep"}  # what the GPU test of a rule runs first
# the lanes' side of the pairs that sit on a total n + m + 2 (the other side takes the rest); - r: the OTHER side is r long
K27_FP_ROWS1 = [160, 150, 97, 1, 120, 33, 159]
K27_FP_ROWS23 = [161, 320, 480, 333]
SS_KEY_ROWS = [160, 150, 97, 1, 161, 480, -100]


def ss_key_rows(mode):
    """(AffineGapLocal holds the query in lanes whatever the lengths: no pair with the long side there)"""
    return [r for r in SS_KEY_ROWS if r > 0 or mode != LOCAL]


def batch_for(case, shape_name):
    """(alphas, betas) of a case on a named shape list -- for AffineGapLocal alpha is the target (the longer side, the window)"""
    return pairs(1000 + sum(map(ord, shape_name)), SHAPES[shape_name], swap=(case.mode == LOCAL))


def batch_total(case, rows=None, seed=77):
    """(alphas, betas) of a case that bounds n + m + 2: every pair exactly at case.total; rows: the lengths of the side the kernels
    hold in lanes (alpha; the query for AffineGapLocal)"""
    return pairs(seed, split_total(case.total, rows), swap=(case.mode == LOCAL))


def n1_pairs(chunk):
    """AffineGapChunk inputs: the batch above on shapes of 1 .. 170 chunk cells, either side the shorter one"""
    return pairs(500 + chunk, [(n * chunk, m * chunk) for n, m in ((60, 60), (50, 50), (30, 70), (20, 90), (61, 58), (55, 57), (170, 165), (90, 120), (120, 40), (1, 30))])


GAP, LOWER = 10, 5  # dna.Gap; a lower-case base is its upper-case code + 5 (gonomics_amd/dna.py)


def n1_groups(chunk):
    """multipleAffineGap inputs: (blocks, every ordered pair of them) -- one- and two-member blocks of A alone and one of C alone
    (a column pair then averages to the table's maximum / minimum times chunkSize), and three blocks of 2 .. 4 members related to
    one root, with substitutions, lower case and gaps (their first member without gaps: no column pair is gap-only)"""
    rng = np.random.default_rng(600 + chunk)
    blocks = [np.full((1, 40 * chunk), A, np.uint8), np.full((2, 37 * chunk), A, np.uint8), np.full((1, 40 * chunk), C, np.uint8)]
    for nseq in (2, 3, 4):
        cells = int(rng.integers(20, 160))
        blk = np.stack([rng.integers(0, 4, size=cells * chunk)] * nseq).astype(np.uint8)
        sub = rng.random(blk.shape) < 0.15
        blk[sub] = rng.integers(0, 4, size=int(sub.sum()))
        blk[rng.random(blk.shape) < 0.3] += LOWER
        blk[rng.random(blk.shape) < 0.1] = GAP
        blk[0, blk[0] == GAP] = C
        blocks.append(blk)
    return blocks, [(x, y) for x in range(len(blocks)) for y in range(len(blocks)) if x != y]


def cells_under_path(alpha, beta, ops):
    """the set of table cells (alpha base, beta base) under the ColM runs of a CIGAR [(run, op)]"""
    i = j = 0
    seen = set()
    for run, op in ops:
        if op == 0:
            seen.update(zip(alpha[i:i + run].tolist(), beta[j:j + run].tolist()))
        if op != 1:
            i += run
        if op != 2:
            j += run
    return seen


def cells_of_batch(res, alphas, betas):
    """cells_under_path over a whole oracle result"""
    _, ops, off = res
    seen = set()
    for p in range(len(alphas)):
        rl = [(int(r), int(o)) for r, o in zip(ops["run_length"][off[p]:off[p + 1]], ops["op"][off[p]:off[p + 1]])]
        seen |= cells_under_path(np.asarray(alphas[p]), np.asarray(betas[p]), rl)
    return seen


def min_reachable(case):
    """whether the table's minimum can lie under an optimal path at all: an isolated mismatch must not cost more than the two gaps
    that avoid it.  (Not so at the lower end of a constant-gap profile rule: there s = 2 * gap - 8 192 < 2 * gap by the rule itself.)"""
    k = case.chunk or 1
    if case.mode == LOCAL and max(flat(case.scores)) < 0:
        return False  # (no column is worth aligning: the query is inserted whole, the target skipped for nothing)
    lo = min(flat(case.scores)) * k
    two_gaps = 2 * (case.gap_open + case.gap_extend * k) if affine(case.mode) else 2 * case.gap_open
    return lo >= two_gaps
