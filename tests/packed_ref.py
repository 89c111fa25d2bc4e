"""The catalogue of tests/test_packed_ref_gpu.py: references, window classes and reads on the block, flag-word and end boundaries of
the packed resident reference.  No GPU in here; tests/test_packed_ref_catalogue_cpu.py asserts that the lists are
what this text says, and checks the numpy restatement of the layout (`pack` / `value`) against the bytes.

The layout (gnx_common.hip.h, KParams): 2 bits per base, 16 bases per dword; one flag bit per 64-base block that holds a byte >= 4, 64
blocks (4 096 bases) per flag word; per flag word the number of flagged blocks before it; per flagged block, in order, the mask of its
N and the mask of its bytes >= 5.

References: `main_ref()` (20 517 bases, a multiple of nothing), `ends_refs()` (twelve lengths on the dword, block and flag-word borders,
three variants each), and the synthetic one (`SYN_LEN`, `SYN_SEED`; `syn_positions()` are the positions the device is asked for).
Window classes: `windows(name)`, named lists of (start, len) on `main_ref()`, generated; `ends_windows(L)` on a reference of `ends`.
`clean_edges` is a class of its own making: see there.
Reads: `reads(name)`: one per window, a third of them mutated copies of a stretch of the window, a third exact copies with the
window's N taken out (the gapless certificate admits those), a third exact copies that keep the N."""
import collections
import functools

import numpy as np

import common

MAIN_LEN = 20517
MAIN_SEED = 4031
N_RUN_WORD = (4090, 4100)     # across the first flag-word border
WORD2 = (8192, 12288)         # flag word 2: the k-th block's N at in-block offset k
N_RUN_BLOCKS = (13000, 13200)  # whole blocks of N
BAD = (16000, 16040)          # bytes 5 .. 10
ENDS_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8191, 8192)
ENDS_VARIANTS = ("clean", "n_last", "n_last_two_and_first")
SYN_LEN, SYN_SEED = 300000500, 77
PASS = 1 << 28                # bases packed per pass of set_reference_packed
MX_NAME, GO, GE = "HumanChimpTwo", -600, -150
RUN_CLASSES = ("start_mod", "end_mod", "beside_n", "all_n", "full_word", "to_the_end", "clean_edges")  # every window of these is GNX_OK


# ---- references ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_ref():
    rng = np.random.default_rng(MAIN_SEED)
    g = rng.integers(0, 4, size=MAIN_LEN).astype(np.uint8)
    g[0] = 4
    g[63] = 4
    g[64] = 4
    g[N_RUN_WORD[0]:N_RUN_WORD[1]] = 4
    for k in range(64):
        g[WORD2[0] + 64 * k + k] = 4
    g[N_RUN_BLOCKS[0]:N_RUN_BLOCKS[1]] = 4
    g[BAD[0]:BAD[1]] = 5 + np.arange(BAD[1] - BAD[0]) % 6
    g[MAIN_LEN - 1] = 4
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def ends_refs():
    """{(length, variant): bytes}"""
    out = collections.OrderedDict()
    for ln in ENDS_LENGTHS:
        for v, variant in enumerate(ENDS_VARIANTS):
            g = np.random.default_rng(1000 * ln + v).integers(0, 4, size=ln).astype(np.uint8)
            if variant == "n_last":
                g[ln - 1] = 4
            elif variant == "n_last_two_and_first":
                g[max(0, ln - 2):] = 4
                g[0] = 4
            g.setflags(write=False)
            out[(ln, variant)] = g
    return out


def syn_positions():
    """positions of the synthetic reference that the read-back asks for: around the 2^28 pass border, around both ends of the N run at
    250 000 000 (before the border), and from 70 bases before the run at 300 000 000 (behind it) to the last base, inside that run"""
    spans = [(PASS - 70, PASS + 71), (250000000 - 70, 250000000 + 71), (250001000 - 70, 250001000 + 71), (300000000 - 70, SYN_LEN)]
    return np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in spans])


def stretches(ref):
    """maximal runs [lo, hi) of bytes that are not A C G T"""
    x = np.concatenate([[0], (np.asarray(ref) >= 4).astype(np.int8), [0]])
    d = np.diff(x)
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


# ---- the layout, restated ----------------------------------------------------------------------------------------------------------------------
Packed = collections.namedtuple("Packed", "n words flags ranks masks")


def pack(ref):
    """the four arrays of the packed form, without the padding words of the library"""
    ref = np.asarray(ref, dtype=np.uint8)
    n = ref.shape[0]
    n_blocks = (n + 63) // 64
    padded = np.zeros(n_blocks * 64, dtype=np.uint8)
    padded[:n] = ref
    two = (padded & 3).astype(np.uint32).reshape(-1, 16)
    words = np.zeros(two.shape[0], dtype=np.uint32)
    for k in range(16):
        words |= two[:, k] << np.uint32(2 * k)
    blocks = padded.reshape(n_blocks, 64)
    flagged = (blocks >= 4).any(axis=1)
    n_fw = (n_blocks + 63) // 64
    fb = np.zeros(n_fw * 64, dtype=bool)
    fb[:n_blocks] = flagged
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    flags = (fb.reshape(n_fw, 64) * weights).sum(axis=1, dtype=np.uint64) if n_fw else np.zeros(0, np.uint64)
    per_word = fb.reshape(n_fw, 64).sum(axis=1)
    ranks = np.concatenate([[0], np.cumsum(per_word)])[:n_fw].astype(np.uint32)
    ex = blocks[flagged]
    masks = np.zeros((ex.shape[0], 2), dtype=np.uint64)
    masks[:, 0] = ((ex == 4) * weights).sum(axis=1, dtype=np.uint64)
    masks[:, 1] = ((ex >= 5) * weights).sum(axis=1, dtype=np.uint64)
    return Packed(n, words, flags, ranks, masks)


def _popcount_below(f, bit):
    return bin(int(f) & ((1 << int(bit)) - 1)).count("1")


def value(p, x):
    """base x as BetaSrcT::value reads it: 0 .. 3, 4 for N, 5 for any byte >= 5"""
    b = (int(p.words[x >> 4]) >> (2 * (x & 15))) & 3
    f = int(p.flags[x >> 12])
    bit = (x >> 6) & 63
    if (f >> bit) & 1:
        e = int(p.ranks[x >> 12]) + _popcount_below(f, bit)
        if (int(p.masks[e, 0]) >> (x & 63)) & 1:
            b = 4
        if (int(p.masks[e, 1]) >> (x & 63)) & 1:
            b = 5
    return b


def values(p):
    """value(p, x) for every x, vectorised"""
    x = np.arange(p.n, dtype=np.int64)
    b = ((p.words[x >> 4] >> (2 * (x & 15)).astype(np.uint32)) & np.uint32(3)).astype(np.uint8)
    f = p.flags[x >> 12] if p.n else np.zeros(0, np.uint64)
    bit = ((x >> 6) & 63).astype(np.uint64)
    on = ((f >> bit) & np.uint64(1)).astype(bool)
    below = f & ((np.uint64(1) << bit) - np.uint64(1))
    pop = np.zeros(p.n, dtype=np.int64)
    for k in range(64):
        pop += ((below >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
    e = p.ranks[x >> 12].astype(np.int64) + pop
    e = np.where(on, e, 0)
    if p.masks.shape[0]:
        inb = (x & 63).astype(np.uint64)
        is_n = on & ((p.masks[e, 0] >> inb) & np.uint64(1)).astype(bool)
        is_bad = on & ((p.masks[e, 1] >> inb) & np.uint64(1)).astype(bool)
        b[is_n] = 4
        b[is_bad] = 5
    return b


def dirty(p, start, length):
    """BetaSrcT::init: a flagged block among those of [start, start + length)"""
    def rank(blk):
        w = blk >> 6
        if w >= p.flags.shape[0]:  # the padding words of the library: no flags, the rank of everything
            return int(p.masks.shape[0])
        return int(p.ranks[w]) + _popcount_below(p.flags[w], blk & 63)
    return rank(((start + length - 1) >> 6) + 1) > rank(start >> 6)


def flagged_blocks(ref):
    return int(pack(ref).masks.shape[0])


# ---- window classes on main ----------------------------------------------------------------------------------------------------------------------
EXACT_LO = 64   # the shortest exact copy, where its window has the room
BESIDE_W = 120  # the longest window beside a stretch; it stops at the neighbouring stretch


def beside(ref, lo, hi):
    """the (up to) four windows beside the stretch [lo, hi), as {name: (start, len)}: `before` ends one base before it, `after` starts
    one base after it (both hold no N and lie in its flagged blocks), `onto` ends on its first base, `from` starts on its last one"""
    st = stretches(ref)
    prev_hi = max([h for _, h in st if h <= lo] + [0])
    next_lo = min([l for l, _ in st if l >= hi] + [len(ref)])
    out = collections.OrderedDict()
    a = max(prev_hi, lo - BESIDE_W)
    if lo - a >= 1:
        out["before"] = (a, lo - a)
        out["onto"] = (a, lo - a + 1)
    b = min(next_lo, hi + BESIDE_W)
    if b - hi >= 1:
        out["after"] = (hi, b - hi)
        out["from"] = (hi - 1, b - hi + 1)
    return out


@functools.lru_cache(maxsize=None)
def windows(name):
    g = main_ref()
    if name == "start_mod":
        return [(s, 300) for s in range(4040, 4104)]
    if name == "end_mod":
        return [(3900, e - 3900) for e in range(4050, 4114)]
    if name == "beside_n":  # (the two of the bad-byte stretch that touch it are in bad_bytes)
        out = []
        for lo, hi in stretches(g):
            for which, w in beside(g, lo, hi).items():
                if (lo, hi) != BAD or which in ("before", "after"):
                    out.append(w)
        return out
    if name == "all_n":
        return [(13000, 1), (13199, 1), (13000, 64), (13056, 64), (13017, 64), (13000, 150), (13050, 150)]
    if name == "full_word":
        return [(8100, 4300), (8192, 4096), (8191, 1000), (11400, 1000)]
    if name == "to_the_end":
        return [(MAIN_LEN - l, l) for l in (1, 16, 64, 65, 300)]
    if name == "clean_edges":
        # windows that touch no flagged block although the block before their first or behind their last base is flagged (`dirty` false:
        # fp_cert_kernel<true> certifies only these), three of them again one base longer on that side (`dirty` true, still no N)
        out = [(4159, 201), (12800, 193), (20280, 201)]
        for l in (200, 250, 300):
            out += [(4160, l), (8192 - l, l), (12288, l), (12992 - l, l), (20480 - l, l)]
        return out
    if name == "bad_bytes":  # every one of these is GNX_EBASE
        b = beside(g, *BAD)
        return [b["onto"], b["from"], (BAD[0], 1), (BAD[1] - 1, 1), (BAD[0] - 100, 300), (BAD[0] + 10, 20), (0, MAIN_LEN)]
    if name == "bad_bytes_ok":  # ... and these two GNX_OK
        return [(BAD[0] - 150, 150), (BAD[1], 150)]
    if name == "every_base":
        return [(x, 1) for x in range(MAIN_LEN) if not BAD[0] <= x < BAD[1]]
    raise KeyError(name)


def ends_windows(ln):
    """the whole reference, its last min(L, 70) bases, its last base"""
    return [(0, ln), (ln - min(ln, 70), min(ln, 70)), (ln - 1, 1)]


# ---- reads --------------------------------------------------------------------------------------------------------------------------------------
def _reads_for(ref, wins, seed, lo, hi):
    rng = np.random.default_rng(seed)
    out = []
    for k, (s, l) in enumerate(wins):
        # inside its window where the window has the room; the exact copies are long where they can be (the certificate's thresholds
        # need about 63 bases under this matrix), the mutated ones of every length
        ln = int(rng.integers(lo if k % 3 == 0 else max(lo, EXACT_LO), hi + 1))
        ln = max(lo, min(ln, l - 2))
        if l >= ln + 2:
            o = s + int(rng.integers(1, l - ln))  # strictly inside: the certificate wants a column on either side
        elif l >= ln:
            o = s + int(rng.integers(0, l - ln + 1))
        else:  # a window shorter than the read: the stretch of the reference around it
            o = min(max(0, s - (ln - l) // 2), max(0, len(ref) - ln))
        src = np.minimum(ref[o:o + ln], 4)
        if len(src) < lo:
            src = np.resize(src, lo)
        kind = k % 3
        if kind == 0:
            r = common.mutate(rng, src, sub=0.05, indel=0.01, geo=0.4, alphabet=4)[:hi]
            if len(r) < lo:  # (the length decides the number of row blocks)
                r = np.concatenate([r, src[:lo - len(r)]])
        elif kind == 1:
            r = np.where(src < 4, src, rng.integers(0, 4, size=len(src))).astype(np.uint8)
        else:
            r = src.copy()
        out.append(np.ascontiguousarray(r, dtype=np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def reads(name, blocks=1):
    """one read per window of the class: 20 .. 150 bases, or 160 .. 330 (two and three row blocks of the fast path) with blocks=2"""
    lo, hi = (20, 150) if blocks == 1 else (161, 330)
    return _reads_for(main_ref(), windows(name), sum(map(ord, name)) * 10 + blocks, lo, hi)


@functools.lru_cache(maxsize=None)
def ends_reads(ln, variant):
    return _reads_for(ends_refs()[(ln, variant)], ends_windows(ln), 7 * ln + ENDS_VARIANTS.index(variant), 20, 150)


@functools.lru_cache(maxsize=None)
def certificate_counts():
    """(admitted, refused) by the host statement of the gapless certificate over the reads of start_mod and beside_n"""
    import os
    from gonomics_amd import _lib
    before = os.environ.get("GNX_DEBUG_ENTRY")
    os.environ["GNX_DEBUG_ENTRY"] = "1"
    try:
        p = _lib.make_params(_lib.GNX_AFFINE_GAP, common.matrices()[MX_NAME], GO, GE)
        g = main_ref()
        ok = [bool(_lib.debug_gapless_certificate(p, r, g[s:s + l])[0]) for name in ("start_mod", "beside_n") for r, (s, l) in zip(reads(name), windows(name))]
    finally:
        if before is None:
            os.environ.pop("GNX_DEBUG_ENTRY", None)
        else:
            os.environ["GNX_DEBUG_ENTRY"] = before
    admitted = sum(ok)
    assert 4 * admitted >= len(ok) and admitted < len(ok), (admitted, len(ok))
    return admitted, len(ok) - admitted
