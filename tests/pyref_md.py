"""The specification of gnx_md_* and gnx_mapq_batch (include/gnx_align.h) restated literally: the CIGAR is expanded into a Python list of
columns and the MD string is built by the walk the header describes, one column at a time.  No run arithmetic, no positions: every GPU
test is byte equality with this."""
import re

from pyref_summary import M, I, D, LOCAL, columns

LETTERS = "ACGTN"
PATTERN = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
INT64_MIN = -(1 << 63)


def md(mode, alpha, beta, route):
    """the MD string of one pair; route = [(run_length, op), ...]; alpha is the described side"""
    cols = columns(route)
    inside = [True] * len(cols)
    if mode == LOCAL:
        k = 0
        while k < len(cols) and cols[k] == D:
            inside[k] = False
            k += 1
        k = len(cols)
        while k > 0 and cols[k - 1] == D:
            k -= 1
            inside[k] = False
    out = []
    i = j = run = 0
    before_is_inside_d = False
    for c, ins in zip(cols, inside):
        if c == M:
            a, b = int(alpha[i]), int(beta[j])
            if ins and a == b:
                run += 1
            elif ins:
                out.append("%d%s" % (run, LETTERS[a]))
                run = 0
            i += 1
            j += 1
        elif c == I:
            j += 1
        else:
            if ins and not before_is_inside_d:
                out.append("%d^%s" % (run, LETTERS[int(alpha[i])]))
                run = 0
            elif ins:
                out.append(LETTERS[int(alpha[i])])
            i += 1
        before_is_inside_d = c == D and ins
    out.append("%d" % run)
    return "".join(out)


def parts(text):
    """(sum of the numbers, letters outside ^ groups, letters inside ^ groups) of an MD string"""
    numbers = sum(int(x) for x in re.findall(r"[0-9]+", text))
    deleted = sum(len(g) - 1 for g in re.findall(r"\^[A-Z]+", text))
    letters = sum(1 for ch in text if ch.isalpha())
    return numbers, letters - deleted, deleted


def mapq(score, second):
    """gnx_mapq_batch's rule on Python integers; second = None (or INT64_MIN): no other candidate"""
    if score <= 0:
        return 0
    s2 = 0 if second is None or second == INT64_MIN or second < 0 else second
    if s2 >= score:
        return 0
    return min(60, (60 * (score - s2)) // score)
