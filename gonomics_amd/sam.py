"""SAM lines from the reports of align.MapReadsReport / align.MapReadPairsReport.

Lines() is text formatting only: every number and letter in a line comes out of the report (the alignment summaries of
gnx_summarize_*, the MD strings of gnx_md_* and the MAPQs of gnx_mapq_batch), none is computed here from bases.  A report made with
tags=True carries md and mapq: the MD string is written on the device, where the resident reference lives, and MAPQ follows the
library's rule (include/gnx_align.h; second_score, its other input, is written as XS).  A report without them gives MAPQ 255 ("not
available") and no MD tag.
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
    """One SAM line (the eleven mandatory fields and the tags AS, NM, MD, XS) per read.  report[r] is the dict of read r; with paired=True
    reads 2k and 2k + 1 are mates.  POS = pos + 1; SEQ and QUAL are in reference orientation (reverse-complemented / reversed on
    strand 1); TLEN is signed, positive on the leftmost mate of a proper pair; NM = n_mismatch + ins_bases + del_bases; MAPQ = the
    report's mapq where a mapped read's dict has one, else 255; MD directly behind NM where the dict has a string under md; XS only where
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
        fields = [names[r], str(flag), ref_name if ok else "*", str(rep["pos"] + 1 if ok else 0), str(rep["mapq"]) if ok and "mapq" in rep else "255", _cigar(rep["xcigar"]) if ok else "*",
                  rnext, str(pnext), str(tlen), _seq(reads[r], reverse), qual]
        if ok:
            fields += ["AS:i:%d" % rep["score"], "NM:i:%d" % (rep["n_mismatch"] + rep["ins_bases"] + rep["del_bases"])]
            if rep.get("md") is not None:
                fields.append("MD:Z:%s" % rep["md"])
            if rep.get("second_score") is not None:
                fields.append("XS:i:%d" % rep["second_score"])
        out.append("\t".join(fields))
    return out
