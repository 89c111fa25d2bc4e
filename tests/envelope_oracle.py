"""The oracle's result for an envelope case (tests/envelope.py) on a batch, computed once and shared by the tests that need it."""
import hashlib

import oracle

_EXPECTED = {}


def _digest(alphas, betas):
    h = hashlib.sha1()
    for x in list(alphas) + list(betas):
        h.update(len(x).to_bytes(8, "little"))
        h.update(bytes(memoryview(x)))
    return h.hexdigest()


def expected(case, key, alphas, betas, ci=10000, threads=8):
    """oracle.align_batch of a case on a batch, once per (case, batch, checkersize) -- the batch itself is part of the key, `key` only
    names it in messages.  Shared: do not change what comes back."""
    k = (case.label, case.mode, tuple(map(tuple, case.scores)), case.gap_open, case.gap_extend, _digest(alphas, betas), ci)
    if k not in _EXPECTED:
        _EXPECTED[k] = oracle.align_batch(case.mode, case.scores, case.gap_open, case.gap_extend, alphas, betas, ci, ci, threads=threads)
    return _EXPECTED[k]
