"""VCF records from the calls of the pile: align.PileupCalls' substitutions and align.PileupIndelCalls' alleles (WriteVcf), or
align.PileupGenotypes' diploid SNP genotypes with a sample column (WriteGenotypeVcf).

WriteVcf() is text formatting only, as sam.Lines() is: which positions are called, with which allele, depth and counts, was decided on
the device by the library's two rules (include/gnx_align.h); the only bases looked up here are the reference letters a VCF record has
to spell out.  Indels stand where the calls put them: nothing is left-normalised here.  Left-aligned records come from normalised calls,
align.PileupIndelCalls(..., normalize=True), which are the same dicts.
"""
import numpy as np

_BASES = "ACGTN"
_ORDER = {"sub": 0, "del": 1, "ins": 2, "long_ins": 2}


def _letters(codes):
    return "".join(_BASES[min(int(c), 4)] for c in codes)


def _indel_record(c, fetch):
    """(POS, REF, ALT, INFO) of one of align.PileupIndelCalls' dicts"""
    kind, x = c["kind"], int(c["pos"])
    info = "DP=%d;AO=%d;AOF=%d" % (c["depth"], c["count"], c["count_fwd"])
    if kind == "del":
        n = int(c["length"])
        if x > 0:
            r = _letters(fetch(x - 1, n + 1))
            return x, r, r[0], info
        r = _letters(fetch(0, n + 1))
        return 1, r, r[-1], info
    if kind == "ins":
        r = _letters(fetch(x, 1))
        return x + 1, r, r + _letters(c["seq"]), info
    if kind == "long_ins":
        return x + 1, _letters(fetch(x, 1)), "<INS>", info + ";SVLEN=%d" % c["length"]
    raise ValueError("WriteVcf: unknown kind %r" % (kind,))


def WriteVcf(out, chrom, ref, sub_calls, indel_calls):
    """Write VCF 4.2 text to `out` (anything with write()) and return the number of records.  ref is the reference as an array of base
    codes, or a callable (start, n) -> the n codes from `start`; sub_calls are align.PileupCalls' dicts, of which only the substitutions
    are written (its "del" and "ins" lines say that there is an indel, the allele calls say which: they replace them); indel_calls are
    align.PileupIndelCalls' dicts.  Records are ordered by POS, then substitutions before deletions before insertions, each class in
    the order it came in.  With x the 0-based position of a call and L its length:
      substitution at x          POS x + 1   REF ref[x]                ALT the alt base
      deletion (x, L), x > 0     POS x       REF ref[x - 1 .. x + L)   ALT ref[x - 1]
      deletion (0, L)            POS 1       REF ref[0 .. L]           ALT ref[L]     (no base before it: anchored behind, as the VCF text asks)
      insertion (x, seq)         POS x + 1   REF ref[x]                ALT ref[x] + seq
      long insertion (x, L)      POS x + 1   REF ref[x]                ALT <INS>      INFO also SVLEN=L (its bases were not kept)
    INFO: DP = depth, AO = count, AOF = count_fwd."""
    fetch = ref if callable(ref) else (lambda start, n: ref[start:start + n])
    head = ["##fileformat=VCFv4.2", "##contig=<ID=%s>" % chrom if callable(ref) else "##contig=<ID=%s,length=%d>" % (chrom, len(ref)),
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth at the position: read bases and deletions over it, both strands">',
            '##INFO=<ID=AO,Number=1,Type=Integer,Description="Reads with exactly this allele">',
            '##INFO=<ID=AOF,Number=1,Type=Integer,Description="Forward-strand share of AO">',
            '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Inserted bases of an <INS> whose sequence was not kept">',
            '##ALT=<ID=INS,Description="Insertion of more than 21 bases">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    records = []
    for c in list(sub_calls) + list(indel_calls):
        kind, x = c["kind"], int(c["pos"])
        info = "DP=%d;AO=%d;AOF=%d" % (c["depth"], c["count"], c["count_fwd"])
        if kind == "sub":
            if "length" in c:
                raise ValueError("WriteVcf: an allele among the substitution calls")
            pos, r, a = x + 1, _letters(fetch(x, 1)), _BASES[int(c["alt"])]
        elif "length" not in c:
            continue  # PileupCalls' own "del" / "ins" line
        else:
            pos, r, a, info = _indel_record(c, fetch)
        records.append((pos, _ORDER[kind], len(records), "\t".join([chrom, str(pos), ".", r, a, ".", ".", info])))
    records.sort(key=lambda rec: rec[:3])
    out.write("\n".join(head + [rec[3] for rec in records]) + "\n")
    return len(records)


def WriteGenotypeVcf(out, chrom, ref, genotypes, indel_calls=(), sample="SAMPLE"):
    """Write VCF 4.2 text with one sample column to `out` and return the number of records.  genotypes are align.PileupGenotypes' dicts,
    indel_calls align.PileupIndelCalls'; ref and the ordering are WriteVcf's, and so are the indel records' POS / REF / ALT / INFO.
    Every conversion from the library's centi-Phred integers is integer arithmetic:
      SNP     POS pos + 1, REF / ALT the two letters, QUAL "%d.%02d" of qual, INFO DP = depth, AO = alt_count, AOF = alt_fwd,
              FORMAT GT:GQ:PL:AD -- GT 0/1 or 1/1, GQ = min(99, (gq + 50) // 100), PL = (pl + 50) // 100 each, AD = ref_count,alt_count
      indel   QUAL ".", FORMAT GT with ./. : the library has no genotype rule for indels (their alleles carry no quality)"""
    fetch = ref if callable(ref) else (lambda start, n: ref[start:start + n])
    head = ["##fileformat=VCFv4.2", "##contig=<ID=%s>" % chrom if callable(ref) else "##contig=<ID=%s,length=%d>" % (chrom, len(ref)),
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="SNP: A C G T read bases over the position, both strands; indel: read bases and deletions over it">',
            '##INFO=<ID=AO,Number=1,Type=Integer,Description="Reads with exactly this allele">',
            '##INFO=<ID=AOF,Number=1,Type=Integer,Description="Forward-strand share of AO">',
            '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Inserted bases of an <INS> whose sequence was not kept">',
            '##ALT=<ID=INS,Description="Insertion of more than 21 bases">',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
            '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Phred-scaled distance to the second best genotype, at most 99">',
            '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype costs, 0 for the called one">',
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read bases of the reference and of the alternative letter">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s" % sample]
    records = []
    for g in genotypes:
        x = int(g["pos"])
        if g["gt"] not in (1, 2):
            raise ValueError("WriteGenotypeVcf: gt %r" % (g["gt"],))
        fields = [chrom, str(x + 1), ".", _letters(fetch(x, 1)), _BASES[int(g["alt"])], "%d.%02d" % (g["qual"] // 100, g["qual"] % 100), ".",
                  "DP=%d;AO=%d;AOF=%d" % (g["depth"], g["alt_count"], g["alt_fwd"]), "GT:GQ:PL:AD",
                  "%s:%d:%s:%d,%d" % ("0/1" if g["gt"] == 1 else "1/1", min(99, (g["gq"] + 50) // 100), ",".join(str((v + 50) // 100) for v in g["pl"]), g["ref_count"], g["alt_count"])]
        records.append((x + 1, 0, len(records), "\t".join(fields)))
    for c in indel_calls:
        pos, r, a, info = _indel_record(c, fetch)
        records.append((pos, _ORDER[c["kind"]], len(records), "\t".join([chrom, str(pos), ".", r, a, ".", ".", info, "GT", "./."])))
    records.sort(key=lambda rec: rec[:3])
    out.write("\n".join(head + [rec[3] for rec in records]) + "\n")
    return len(records)


def LettersToBases(text):
    """the base codes of an ALT's inserted letters (what align.PileupAlleles gives as seq)"""
    return np.asarray([_BASES.index(ch) for ch in text], dtype=np.uint8)
