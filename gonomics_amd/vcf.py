"""VCF records from the calls of the pile: align.PileupCalls' substitutions and align.PileupIndelCalls' alleles.

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
        elif kind == "del":
            n = int(c["length"])
            if x > 0:
                r = _letters(fetch(x - 1, n + 1))
                pos, a = x, r[0]
            else:
                r = _letters(fetch(0, n + 1))
                pos, a = 1, r[-1]
        elif kind == "ins":
            r = _letters(fetch(x, 1))
            pos, a = x + 1, r + _letters(c["seq"])
        elif kind == "long_ins":
            pos, r, a = x + 1, _letters(fetch(x, 1)), "<INS>"
            info += ";SVLEN=%d" % c["length"]
        else:
            raise ValueError("WriteVcf: unknown kind %r" % (kind,))
        records.append((pos, _ORDER[kind], len(records), "\t".join([chrom, str(pos), ".", r, a, ".", ".", info])))
    records.sort(key=lambda rec: rec[:3])
    out.write("\n".join(head + [rec[3] for rec in records]) + "\n")
    return len(records)


def LettersToBases(text):
    """the base codes of an ALT's inserted letters (what align.PileupAlleles gives as seq)"""
    return np.asarray([_BASES.index(ch) for ch in text], dtype=np.uint8)
