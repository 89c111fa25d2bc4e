"""SAM lines from the reports of align.MapReadsReport / align.MapReadPairsReport.

Lines() is text formatting only: every number in a line comes out of the report (the alignment summaries of gnx_summarize_*), none
is computed here from bases.  The MD tag is not written: it needs the target's bases on the host, and the resident reference lives
on the device.  MAPQ is 255 ("not available"): the library defines no MAPQ formula (second_score is its raw ingredient, written as XS).
"""
import numpy as np

from . import align
from . import dna

_BASES = "ACGTN"
FLAG_PAIRED, FLAG_PROPER, FLAG_UNMAPPED, FLAG_MATE_UNMAPPED, FLAG_REVERSE, FLAG_MATE_REVERSE, FLAG_FIRST, FLAG_SECOND = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80


def _mapped(rep):
    return rep["best"] >= 0 and rep["pos"] is not None


def _cigar(xcigar):
    """the extended CIGAR without the free end D runs of the mapping mode (SAM anchors the alignment at POS instead)"""
    runs = list(xcigar)
    if runs and runs[0][1] == align.ColD:
        runs = runs[1:]
    if runs and runs[-1][1] == align.ColD:
        runs = runs[:-1]
    return align.FormatXCigar(runs)


def _seq(read, reverse):
    b = np.array(read, dtype=np.uint8)
    if reverse:
        dna.ReverseComplement(b)
    return "".join(_BASES[int(x)] for x in b) or "*"


def Lines(names, reads, report, ref_name, quals=None, paired=False):
    """One SAM line (the eleven mandatory fields and the tags AS, NM, XS) per read.  report[r] is the dict of read r; with paired=True
    reads 2k and 2k + 1 are mates.  POS = pos + 1; SEQ and QUAL are in reference orientation (reverse-complemented / reversed on
    strand 1); TLEN is signed, positive on the leftmost mate of a proper pair; NM = n_mismatch + ins_bases + del_bases; XS only where
    the report has a second_score.  An unmapped read has RNAME *, POS 0, MAPQ 255, CIGAR * and no tags."""
    out = []
    for r, rep in enumerate(report):
        ok = _mapped(rep)
        reverse = ok and rep["strand"] == 1
        flag = (0 if ok else FLAG_UNMAPPED) | (FLAG_REVERSE if reverse else 0)
        rnext, pnext, tlen = "*", 0, 0
        if paired:
            mate = report[r ^ 1]
            mate_ok = _mapped(mate)
            flag |= FLAG_PAIRED | (FLAG_FIRST if r % 2 == 0 else FLAG_SECOND)
            flag |= FLAG_PROPER if ok and mate_ok and rep.get("proper") else 0
            flag |= 0 if mate_ok else FLAG_MATE_UNMAPPED
            flag |= FLAG_MATE_REVERSE if mate_ok and mate["strand"] == 1 else 0
            if mate_ok:
                rnext, pnext = ("=" if ok else ref_name), mate["pos"] + 1
            if ok and mate_ok and rep.get("proper"):
                leftmost = rep["pos"] < mate["pos"] or (rep["pos"] == mate["pos"] and r % 2 == 0)
                tlen = rep["tlen"] if leftmost else -rep["tlen"]
        qual = "*"
        if quals is not None:
            qual = quals[r][::-1] if reverse else quals[r]
        fields = [names[r], str(flag), ref_name if ok else "*", str(rep["pos"] + 1 if ok else 0), "255", _cigar(rep["xcigar"]) if ok else "*",
                  rnext, str(pnext), str(tlen), _seq(reads[r], reverse), qual]
        if ok:
            fields += ["AS:i:%d" % rep["score"], "NM:i:%d" % (rep["n_mismatch"] + rep["ins_bases"] + rep["del_bases"])]
            if rep.get("second_score") is not None:
                fields.append("XS:i:%d" % rep["second_score"])
        out.append("\t".join(fields))
    return out
