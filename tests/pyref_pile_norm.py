"""The specification of gnx_pileup_alleles_norm / gnx_pileup_indel_calls_norm (include/gnx_align.h) restated literally: the rule's two
loops move an allele one base at a time on Python lists, and `normalized` merges a pyref_pile_alleles dict allele by allele.  No chunk,
no closed form, no rotation: every GPU test is equality with this.  Calls go through pyref_pile_alleles.calls unchanged."""
import pyref_pile_alleles as ref

DEL, INS, LONG_INS = ref.DEL, ref.INS, ref.LONG_INS


def unpack(key):
    """the digits of a packed inserted sequence as base codes (a read N: 4)"""
    out = []
    while key:
        out.append(key % 8 - 1)
        key //= 8
    return out


def shift_deletion(R, x, L, lo):
    """R: the reference codes from position 0 on (4 = N).  -> the new x"""
    while x - 1 >= lo and R[x - 1] < 4 and R[x - 1] == R[x + L - 1]:
        x -= 1
    return x


def shift_insertion(R, x, s, lo):
    """s: the inserted base codes behind x.  -> (the new x, the new s)"""
    s = list(s)
    while x - 1 >= lo and R[x] < 4 and s[-1] < 4 and R[x] == s[-1]:
        s = [int(R[x])] + s[:-1]
        x -= 1
    return x, s


def normalize(R, pos, kind, key, lo):
    """one allele (pos, kind, key) of pyref_pile_alleles -> the normalised (pos, kind, key)"""
    if kind == DEL:
        return shift_deletion(R, pos, key, lo), DEL, key
    if kind == INS:
        x, s = shift_insertion(R, pos, unpack(key), lo)
        return x, INS, ref.pack(s)
    return pos, kind, key


def normalized(alleles, ref_codes, region):
    """a pyref_pile_alleles dict {(pos, kind, key): [fwd, rev]} -> the dict of the normalised alleles, counts summed where they merge.
    ref_codes[k] is the code of reference position k; region = (region_start, region_len)."""
    out = ref.new_alleles()
    for (pos, kind, key), (f, r) in alleles.items():
        c = out.setdefault(normalize(ref_codes, pos, kind, key, region[0]), [0, 0])
        c[0] += f
        c[1] += r
    return out
