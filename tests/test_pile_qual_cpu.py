"""The quality pile and the genotype rule without a GPU: the symbols and struct layouts, the restatement (tests/pyref_pile_qual.py) on the
header's worked values and on a hand-made pile, geno_rule.h compiled for the CPU against the restatement over random and edge vectors,
the argument checks that need no device, the resources of the new kernels, WriteGenotypeVcf's text, and the C++ mirror's build."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest

import pileup_cases as pc
import pyref_pile_qual as ref
from gonomics_amd import _lib, align, dna, vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pile_qual_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "pile_qual_mirror_test.bin")
RULE_SRC = os.path.join(ROOT, "tests", "cpp", "geno_rule_test.cpp")
RULE_BIN = os.path.join(ROOT, "tests", "cpp", "geno_rule_test.bin")
NAMES = ("gnx_pileup_track_qualities", "gnx_pileup_qual_info", "gnx_pileup_add_by_offset_qual", "gnx_pileup_get_qual", "gnx_pileup_genotypes")
SENTINEL = 0x5A5A5A5A5A5A5A5A
SAT = 2 ** 31 - 1


def _built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


# ---- 1. symbols and layouts ----
def test_symbols_and_structs(tmp_path):
    _built()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for nm in NAMES:
        assert hasattr(L, nm) and nm in _lib.EXPORTS
    for nm in ("PileupTrackQualities", "PileupQualInfo", "PileupGetQual", "PileupGenotypes"):
        assert callable(getattr(align, nm))
    assert callable(vcf.WriteGenotypeVcf)
    assert ctypes.sizeof(_lib.GnxGenoOpts) == 24 and _lib.PILE_GENOTYPE_DTYPE.itemsize == 48
    want = {"pos": 0, "pl": 8, "gq": 20, "qual": 24, "depth": 28, "ref_count": 32, "alt_count": 36, "alt_fwd": 40, "gt": 44, "ref": 45, "alt": 46, "_pad": 47}
    assert {f: _lib.PILE_GENOTYPE_DTYPE.fields[f][1] for f in want} == want
    # the C compiler's view of both structs
    prog = str(tmp_path / "sizeof.bin")
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "gnx_align.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(gnx_geno_opts), sizeof(gnx_pile_genotype), ' \
           'offsetof(gnx_pile_genotype, gq), offsetof(gnx_pile_genotype, alt_fwd), offsetof(gnx_pile_genotype, gt)); return 0; }\n'
    subprocess.run(["gcc", "-x", "c", "-I" + os.path.join(ROOT, "include"), "-o", prog, "-"], input=code, text=True, check=True)
    assert subprocess.run([prog], capture_output=True, text=True, check=True).stdout.split() == ["24", "48", "20", "40", "44"]
    assert _lib.QUAL_MAX_READS == 23091222


# ---- 2. the restatement: the worked values of the header and a hand-made pile ----
def _uniform(c, b, n_ref, n_alt, q):
    fwd, Q = [0] * 4, [0] * 4
    fwd[c], fwd[b], Q[c], Q[b] = n_ref, n_alt, n_ref * q, n_alt * q
    return fwd, [0] * 4, Q


def test_restatement_worked_genotypes():
    o = ref.opts()
    fwd, rev, Q = _uniform(0, 2, 10, 10, 30)
    assert ref.costs(fwd, Q, 0, o) == (2, [34770, 9020, 38070])
    g = ref.genotype(fwd, rev, Q, 0, o)
    assert (g["gt"], g["qual"], g["gq"], g["pl"], g["alt"], g["depth"], g["ref_count"], g["alt_count"]) == (1, 25750, 25750, [25750, 0, 29050], 2, 20, 10, 10)
    fwd, rev, Q = _uniform(0, 2, 19, 1, 30)
    assert ref.costs(fwd, Q, 0, o)[1][:2] == [3477, 9020] and ref.genotype(fwd, rev, Q, 0, o) is None
    fwd, rev, Q = _uniform(0, 2, 17, 3, 30)
    assert ref.costs(fwd, Q, 0, o) == (2, [10431, 9020, 62409])
    g = ref.genotype(fwd, rev, Q, 0, o)
    assert (g["gt"], g["qual"]) == (1, 1411)
    # twenty q2 alt bases against ten q40 ref bases: no alt / alt call
    fwd, rev, Q = _uniform(1, 3, 10, 20, 0)
    Q[1], Q[3] = 400, 40
    assert ref.costs(fwd, Q, 1, o) == (3, [13540, 12030, 48070])
    # all alt: alt / alt
    g = ref.genotype([0, 0, 0, 12], [0] * 4, [0, 0, 0, 360], 0, o)
    assert (g["gt"], g["alt"], g["pl"]) == (2, 3, [36000 + 5724 - 3300, 301 * 12 + 3000 - 3300, 0])
    assert ref.genotype([0, 0, 0, 12], [0] * 4, [0, 0, 0, 360], 4, o) is None  # a reference N is silent


HAND_QUALS = [30, 30, 10, 30, 40, 30, 5, 30, 30]  # min_baseq 20 cuts the G at 102 (q10) and the T at 107 (q5)


def test_restatement_hand_made_pile():
    read, route, where = pc.WORKED[0]
    assert (pc.ALPHA, pc.ALPHA_AT, read, route) == ("ACGTACGTAC", 100, "ACGAACTAC", [(6, pc.M), (1, pc.D), (3, pc.M)])
    for strand in (0, 1):
        pile = ref.add(ref.new_pile(10), pc.LOCAL, 100, dna.StringToBases(read), HAND_QUALS, strand, route, (100, 10), 20)
        base = {100: "A", 101: "C", 103: "A", 104: "A", 105: "C", 108: "A", 109: "C"}
        qsum = {100: (0, 30), 101: (1, 30), 103: (0, 30), 104: (0, 40), 105: (1, 30), 108: (0, 30), 109: (1, 30)}
        for k, row in enumerate(pile):
            x = 100 + k
            exp = [[0] * 5, [0] * 5]
            if x in base:
                exp[strand][pc.CODE[base[x]]] = 1
            q = [0] * 4
            if x in qsum:
                q[qsum[x][0]] = qsum[x][1]
            assert row["base"] == exp and row["qsum"] == q and row["del"][strand] == (1 if x == 106 else 0) and row["ins"] == [0, 0], x
        # min_baseq 0: the counts are the plain pile's, the qualities all there; a byte above 93 counts as 93; a read N has no sum
        pile = ref.add(ref.new_pile(10), pc.LOCAL, 100, dna.StringToBases(read), HAND_QUALS, strand, route, (100, 10), 0)
        plain = pc.worked_pile(where, strand, (100, 10))
        assert [(r["base"], r["del"], r["ins"]) for r in pile] == [(r["base"], r["del"], r["ins"]) for r in plain]
        assert pile[2]["qsum"] == [0, 0, 10, 0] and pile[7]["qsum"] == [0, 0, 0, 5]
    pile = ref.add(ref.new_pile(3), pc.LOCAL, 0, [0, 4, 1], [200, 50, 94], 0, [(3, pc.M)], (0, 3), 93)
    assert [r["qsum"] for r in pile] == [[93, 0, 0, 0], [0] * 4, [0, 93, 0, 0]] and [r["base"][0] for r in pile] == [[1, 0, 0, 0, 0], [0] * 5, [0, 1, 0, 0, 0]]


# ---- 3. geno_rule.h, compiled for the CPU, against the restatement ----
def _rule_vectors():
    """(fwd[4], rev[4], Q[4], c, opts) vectors: seeded random ones, then the edges of the rule"""
    rng = np.random.default_rng(2028)
    out = []
    for k in range(4000):
        hi = (4, 40, 3000)[k % 3]
        fwd, rev = rng.integers(0, hi, 4).tolist(), rng.integers(0, hi, 4).tolist()
        Q = [int(rng.integers(0, 94 * (f + r) + 1)) for f, r in zip(fwd, rev)]
        o = ref.opts(int(rng.integers(1, 30)), int(rng.integers(0, 3000)), int(rng.integers(0, (1 << 20) + 1)) if k % 5 == 0 else 3000, int(rng.integers(0, (1 << 20) + 1)) if k % 5 == 0 else 3300)
        out.append((fwd, rev, Q, int(rng.integers(0, 5)), o))
    o = ref.opts()
    z = [0] * 4
    # ties in the choice of b: two and three letters with the same E (equal E from different n and Q: 477 * 100 = 100 * 477), every reference
    for c in range(4):
        others = [a for a in range(4) if a != c]
        for tied in ([others[0], others[1]], [others[1], others[2]], [others[0], others[2]], others):
            fwd, Q = [0] * 4, [0] * 4
            for a in tied:
                fwd[a], Q[a] = 6, 180
            fwd[c], Q[c] = 5, 150
            out.append((fwd, z, Q, c, o))
        fwd, Q = [0] * 4, [0] * 4
        fwd[others[0]], Q[others[0]] = 100, 0        # E = 47 700
        fwd[others[2]], Q[others[2]] = 0, 477        # E = 47 700 from the qualities alone
        out.append((fwd, z, Q, c, o))
    # ties in the choice of g: L0 == L1 < L2, L1 == L2 < L0, L0 == L2 < L1, all three equal (priors chosen for it)
    fwd, Q = [10, 0, 10, 0], [300, 0, 300, 0]                  # E = 34 770 both, 301 * 20 = 6 020
    out.append((fwd, z, Q, 0, ref.opts(prior_het=34770 - 6020, prior_hom=5000)))   # L = (34770, 34770, 39770): g = 0
    out.append((fwd, z, Q, 0, ref.opts(prior_het=34770 - 6020 - 1, prior_hom=5000)))  # one less: g = 1, qual 1
    out.append((fwd, z, Q, 0, ref.opts(prior_het=5000, prior_hom=0)))              # L = (34770, 11020, 34770): L0 == L2
    out.append((fwd, z, Q, 0, ref.opts(prior_het=40000, prior_hom=0)))             # L = (34770, 46020, 34770): g = 0 by the tie
    out.append(([0, 0, 10, 0], z, [0, 0, 300, 0], 0, ref.opts(prior_het=0, prior_hom=3010)))  # L = (34770, 3010, 3010): g = 1 by the tie
    out.append(([0, 0, 10, 0], z, [0, 0, 300, 0], 0, ref.opts(prior_het=1, prior_hom=3010)))  # g = 2
    out.append(([1, 0, 1, 0], z, [0, 0, 0, 0], 0, ref.opts(prior_het=0, prior_hom=0)))        # L = (477, 602, 477)
    out.append((z, z, z, 0, ref.opts(prior_het=0, prior_hom=0)))                              # all three equal at depth 0
    # n[b] == 0 (nothing but reference bases; nothing at all), c's count 0
    out.append(([9, 0, 0, 0], [8, 0, 0, 0], [500, 0, 0, 0], 0, o))
    out.append(([0, 0, 0, 7], [0, 0, 0, 8], [0, 0, 0, 450], 1, o))
    out.append(([0, 0, 0, 7], [0, 0, 0, 8], [0, 0, 0, 0], 1, o))  # (bases of quality 0 still cost 477 each)
    # depth == min_depth - 1 and == min_depth; qual == min_qual - 1 and == min_qual (10 + 10 at q30: qual 25 750)
    fwd, rev, Q = [6, 0, 5, 0], [4, 0, 5, 0], [300, 0, 300, 0]
    for md, mq in ((20, 0), (21, 0), (1, 25750), (1, 25751), (20, 25750), (21, 25750)):
        out.append((fwd, rev, Q, 0, ref.opts(md, mq)))
    out.append((fwd, rev, Q, 0, ref.opts(1, SAT)))
    # counts and sums at 2^31 - 1: the 64-bit products, the saturation of pl / gq / qual, of depth and of the counts
    out.append(([SAT, 0, SAT, 0], z, [SAT, 0, SAT, 0], 0, o))
    out.append(([SAT, 0, SAT, 0], [SAT, 0, SAT, 0], [SAT, 0, SAT, 0], 0, o))
    out.append(([0, SAT, 0, 0], [0, SAT, 0, 0], [0, SAT, 0, 0], 0, ref.opts(SAT, SAT, 1 << 20, 1 << 20)))
    out.append(([0, SAT, 0, 0], z, [0, SAT, 0, 0], 3, ref.opts(SAT, SAT, 0, 0)))
    out.append(([SAT, SAT, SAT, SAT], [SAT, SAT, SAT, SAT], [SAT, SAT, SAT, SAT], 2, o))
    out.append(([1, 0, SAT, 0], z, [0, 0, 93, 0], 0, o))
    out.append(([SAT, 0, 5, 0], z, [0, 0, 5 * 93, 0], 0, o))
    out.append(([100, 0, 22470000, 0], z, [3000, 0, SAT, 0], 0, o))
    # a reference N, whatever lies over it
    out.append(([0, 50, 0, 0], [0, 50, 0, 0], [0, 3000, 0, 0], 4, o))
    return out


def _line(rec):
    return "none" if rec is None else " ".join(str(v) for v in [rec["gt"], rec["alt"]] + rec["pl"] + [rec["gq"], rec["qual"], rec["depth"], rec["ref_count"], rec["alt_count"], rec["alt_fwd"]])


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_geno_rule_header_against_the_restatement(flags):
    binary = RULE_BIN if flags == ("-O2",) else RULE_BIN.replace(".bin", "_san.bin")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "gonomics_amd", "csrc"), "-o", binary, RULE_SRC])
    vectors = _rule_vectors()
    text = "".join(" ".join(str(v) for v in fwd + rev + Q + [c, o["min_depth"], o["min_qual"], o["prior_het"], o["prior_hom"]]) + "\n" for fwd, rev, Q, c, o in vectors)
    got = subprocess.run([binary], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    want = [_line(ref.genotype(fwd, rev, Q, c, o)) for fwd, rev, Q, c, o in vectors]
    assert len(got) == len(want)
    bad = [(vectors[k], got[k], want[k]) for k in range(len(want)) if got[k] != want[k]]
    assert not bad, bad[:3]
    # conditions on the inputs: every genotype, every alternative, records and silence, saturated values
    recs = [w.split() for w in want if w != "none"]
    assert {r[0] for r in recs} == {"1", "2"} and {r[1] for r in recs} == {"0", "1", "2", "3"} and 500 < len(recs) < len(want) - 500
    assert any(str(SAT) in r[2:7] for r in recs) and any(r[7] == str(SAT) for r in recs)


# ---- 4. argument checks need no device ----
def _geno_rc(o, give_out=True, give_n=True):
    recs, n = ctypes.c_void_p(SENTINEL), ctypes.c_int64(SENTINEL)
    rc = _lib.lib().gnx_pileup_genotypes(ctypes.byref(o) if o is not None else None, ctypes.byref(recs) if give_out else None, ctypes.byref(n) if give_n else None)
    assert recs.value == SENTINEL and n.value == SENTINEL  # nothing was written
    return rc


@pytest.mark.parametrize("bad", [(0, 0, 3000, 3300), (-1, 0, 3000, 3300), (1, -1, 3000, 3300), (1, 0, -1, 3300), (1, 0, (1 << 20) + 1, 3300), (1, 0, 3000, -1), (1, 0, 3000, (1 << 20) + 1)], ids=str)
def test_genotype_options_out_of_range(bad):
    _lib.check(_lib.lib().gnx_pileup_close())
    assert _geno_rc(_lib.GnxGenoOpts(*bad)) == _lib.GNX_EINVAL
    assert b"no open pile" not in _lib.lib().gnx_last_error()


def test_entries_without_a_pile():
    L = _lib.lib()
    _lib.check(L.gnx_pileup_close())
    assert _geno_rc(None) == _lib.GNX_EINVAL and _geno_rc(_lib.GnxGenoOpts(1, 0, 0, 1 << 20), give_out=False) == _lib.GNX_EINVAL
    assert _geno_rc(_lib.GnxGenoOpts(1, 0, 0, 1 << 20), give_n=False) == _lib.GNX_EINVAL
    assert _geno_rc(_lib.GnxGenoOpts(1, 0, 0, 1 << 20)) == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()  # in range: refused for the missing pile
    for q in (0, 93, 94, -1):
        assert L.gnx_pileup_track_qualities(q) == _lib.GNX_EINVAL
    info = np.full(3, SENTINEL, dtype=np.int64)
    assert L.gnx_pileup_qual_info(info.ctypes.data, info.ctypes.data + 8, info.ctypes.data + 16) == _lib.GNX_EINVAL and (info == SENTINEL).all()
    assert L.gnx_pileup_qual_info(None, None, None) == _lib.GNX_EINVAL
    rows = np.full(4, SENTINEL, dtype=np.int64)
    assert L.gnx_pileup_get_qual(0, 1, rows.ctypes.data) == _lib.GNX_EINVAL and (rows == SENTINEL).all()
    p = _lib.make_params(_lib.GNX_AFFINE_GAP_LOCAL, align.HumanChimpTwoScoreMatrix, -600, -150)
    for call in (lambda: align.PileupTrackQualities(), lambda: align.PileupQualInfo(), lambda: align.PileupGetQual(), lambda: align.PileupGenotypes(1),
                 lambda: align.PileupAdd(p, [[0]], [(0, 1)], [0], [[(1, 0)]], quals=[[30]])):
        with pytest.raises(_lib.GnxError) as ei:
            call()
        assert ei.value.code == _lib.GNX_EINVAL


def test_add_qual_argument_errors_need_no_device():
    import test_pileup_cpu as tpc
    L = _lib.lib()
    _lib.check(L.gnx_pileup_close())

    def run(c, qual):
        return L.gnx_pileup_add_by_offset_qual(None if "p" in c.null else ctypes.byref(c.p), c.n, c.ptr("cat"), c.ptr("off"), c.ptr("start"), c.ptr("len"),
                                               c.ptr("strand"), c.ptr("ops"), c.ptr("ooff"), c.ptr("use"), qual)
    for what in sorted(tpc.ADD_BREAKS):
        c = tpc._Add()
        tpc.ADD_BREAKS[what](c)
        quals = np.full(c.cat.shape[0], 30, np.uint8)
        assert run(c, quals.ctypes.data) == _lib.GNX_EINVAL, what
        assert b"no open pile" not in L.gnx_last_error(), what
    c = tpc._Add()
    assert run(c, None) == _lib.GNX_EINVAL and b"qual_cat" in L.gnx_last_error()  # a null qual_cat with n_pairs > 0
    assert run(c, np.full(c.cat.shape[0], 30, np.uint8).ctypes.data) == _lib.GNX_EINVAL and b"no open pile" in L.gnx_last_error()
    with pytest.raises(ValueError):
        align.PileupAdd(c.p, [[0, 1]], [(0, 2)], [0], [[(2, 0)]], quals=[[30]])  # one quality per base
    with pytest.raises(ValueError):
        align.PileupAdd(c.p, [[0, 1]], [(0, 2)], [0], [[(2, 0)]], quals=[" I"])  # a character below '!'
    assert align._phred("!I~").tolist() == [0, 40, 93] and align._phred(np.array([0, 40, 200])).tolist() == [0, 40, 200]


# ---- 5. kernel resources, from the gfx950 code object inside the built library ----
# name -> (VGPRs, LDS bytes) as built
QUAL_PINS = {"qual_add_kernel": (80, 0), "geno_call_kernel<false>": (96, 0), "geno_call_kernel<true>": (115, 0)}


def test_qual_kernel_resources(tmp_path):
    import test_kernel_resources as tkr
    if not os.path.exists(f"{tkr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    kernels = tkr._kernels(tmp_path)
    mine = {n: k for n, k in kernels.items() if n.startswith(("qual_", "geno_"))}
    assert sorted(mine) == sorted(QUAL_PINS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)   # no scratch, no spills
        assert k["agpr_count"] == 0, (name, k)
        assert tkr._waves_per_simd(k) >= 4, (name, k["vgpr_count"])
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == QUAL_PINS[name], (name, k)


# ---- 6. WriteGenotypeVcf ----
def test_write_genotype_vcf_text():
    genome = dna.StringToBases("ACGTACGTACGTAAAACCCC")
    genos = [{"pos": 9, "gt": 2, "ref": 1, "alt": 3, "pl": [41724, 3312, 0], "gq": 3312, "qual": 41724, "depth": 12, "ref_count": 0, "alt_count": 12, "alt_fwd": 5},
             {"pos": 2, "gt": 1, "ref": 2, "alt": 0, "pl": [25750, 0, 29050], "gq": 25750, "qual": 25750, "depth": 20, "ref_count": 10, "alt_count": 10, "alt_fwd": 7},
             {"pos": 5, "gt": 1, "ref": 1, "alt": 3, "pl": [1411, 0, 53389], "gq": 1411, "qual": 1411, "depth": 21, "ref_count": 17, "alt_count": 3, "alt_fwd": 0},
             {"pos": 6, "gt": 1, "ref": 2, "alt": 1, "pl": [49, 0, 150], "gq": 49, "qual": 49, "depth": 4, "ref_count": 2, "alt_count": 2, "alt_fwd": 1},
             {"pos": 7, "gt": 1, "ref": 3, "alt": 1, "pl": [SAT, 0, 50], "gq": 50, "qual": SAT, "depth": 4, "ref_count": 2, "alt_count": 2, "alt_fwd": 1}]
    indels = [{"pos": 5, "kind": "ins", "length": 2, "seq": np.array([3, 3], np.uint8), "count": 4, "count_fwd": 2, "depth": 9, "ref": 1},
              {"pos": 3, "kind": "del", "length": 2, "seq": None, "count": 5, "count_fwd": 5, "depth": 8, "ref": 3}]
    out = io.StringIO()
    assert vcf.WriteGenotypeVcf(out, "chr1", genome, genos, indels, sample="S1") == 7
    head = ["##fileformat=VCFv4.2", "##contig=<ID=chr1,length=20>",
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="SNP: A C G T read bases over the position, both strands; indel: read bases and deletions over it">',
            '##INFO=<ID=AO,Number=1,Type=Integer,Description="Reads with exactly this allele">',
            '##INFO=<ID=AOF,Number=1,Type=Integer,Description="Forward-strand share of AO">',
            '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Inserted bases of an <INS> whose sequence was not kept">',
            '##ALT=<ID=INS,Description="Insertion of more than 21 bases">',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Phred-scaled distance to the second best genotype, at most 99">',
            '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype costs, 0 for the called one">',
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read bases of the reference and of the alternative letter">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    body = ["chr1\t3\t.\tG\tA\t257.50\t.\tDP=20;AO=10;AOF=7\tGT:GQ:PL:AD\t0/1:99:258,0,291:10,10",
            "chr1\t3\t.\tGTA\tG\t.\t.\tDP=8;AO=5;AOF=5\tGT\t./.",
            "chr1\t6\t.\tC\tT\t14.11\t.\tDP=21;AO=3;AOF=0\tGT:GQ:PL:AD\t0/1:14:14,0,534:17,3",
            "chr1\t6\t.\tC\tCTT\t.\t.\tDP=9;AO=4;AOF=2\tGT\t./.",
            "chr1\t7\t.\tG\tC\t0.49\t.\tDP=4;AO=2;AOF=1\tGT:GQ:PL:AD\t0/1:0:0,0,2:2,2",
            "chr1\t8\t.\tT\tC\t21474836.47\t.\tDP=4;AO=2;AOF=1\tGT:GQ:PL:AD\t0/1:1:21474836,0,1:2,2",
            "chr1\t10\t.\tC\tT\t417.24\t.\tDP=12;AO=12;AOF=5\tGT:GQ:PL:AD\t1/1:33:417,33,0:0,12"]
    assert out.getvalue() == "\n".join(head + body) + "\n"
    # no records; a callable reference; WriteVcf's text is what it was
    out = io.StringIO()
    assert vcf.WriteGenotypeVcf(out, "c", lambda s, n: genome[s:s + n], []) == 0 and out.getvalue().split("\n")[1] == "##contig=<ID=c>" and out.getvalue().endswith("\tFORMAT\tSAMPLE\n")
    out = io.StringIO()
    assert vcf.WriteVcf(out, "chr1", genome, [], indels) == 2
    assert out.getvalue().split("\n")[-3:] == ["chr1\t3\t.\tGTA\tG\t.\t.\tDP=8;AO=5;AOF=5", "chr1\t6\t.\tC\tCTT\t.\t.\tDP=9;AO=4;AOF=2", ""]


# ---- 7. the C++ mirror ----
def _build_cpp():
    _built()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC, _lib.LIB_PATH,
                           "-Wl,-rpath," + os.path.join(ROOT, "gonomics_amd"), "-L/opt/rocm/lib", "-lamdhip64"])


def test_cpp_pile_qual_mirror_builds_and_refuses_without_gpu():
    _build_cpp()
    assert subprocess.call([BIN]) in (0, 2)  # 2 == "no HIP device" (no CPU fallback); 0 on a GPU box
