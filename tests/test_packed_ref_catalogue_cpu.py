"""The catalogue of tests/packed_ref.py is what its text says (a class that silently shrinks fails here), and the numpy restatement of
the packed layout -- words, flags, ranks, masks, value(x) by rank and mask -- gives back the bytes of every reference of the catalogue."""
import numpy as np
import pytest

import packed_ref as pr


def test_main_reference_holds_its_exceptions():
    g = pr.main_ref()
    assert len(g) == pr.MAIN_LEN == 20517 and all(pr.MAIN_LEN % k for k in (16, 64, 4096))
    assert g[0] == 4 and g[63] == 4 and g[64] == 4 and g[62] < 4 and g[65] < 4 and g[-1] == 4 and g[-2] < 4
    assert (g[4090:4100] == 4).all() and g[4089] < 4 and g[4100] < 4
    assert (g[13000:13200] == 4).all() and g[12999] < 4 and g[13200] < 4
    assert sorted(set(g[16000:16040].tolist())) == [5, 6, 7, 8, 9, 10] and g[15999] < 4 and g[16040] < 4
    st = pr.stretches(g)
    assert len(st) == 1 + 1 + 1 + 64 + 1 + 1 + 1 and st[0] == (0, 1) and st[1] == (63, 65) and st[-1] == (20516, 20517)
    assert np.flatnonzero(g >= 5).tolist() == list(range(16000, 16040))


def test_flag_word_2_has_64_flagged_blocks():
    g = pr.main_ref()
    p = pr.pack(g)
    assert int(p.flags[2]) == (1 << 64) - 1 and int(p.ranks[3]) - int(p.ranks[2]) == 64
    for k in range(64):
        blk = g[8192 + 64 * k:8192 + 64 * (k + 1)]
        assert np.flatnonzero(blk >= 4).tolist() == [k]
    assert int(p.flags[0]) & 3 == 3 and (int(p.flags[0]) >> 63) & 1 and int(p.flags[1]) & 1  # blocks 0, 1, 63 and 64
    assert bin(int(p.flags[3])).count("1") == (13199 // 64 - 13000 // 64 + 1) + 1  # the N run's blocks, and the block of the bad bytes
    whole = [b for b in range(13000 // 64, 13200 // 64 + 1) if (g[64 * b:64 * b + 64] == 4).all()]
    assert len(whole) == 2  # blocks that are N and nothing else


def test_ends_lengths_and_variants():
    refs = pr.ends_refs()
    assert sorted({k[0] for k in refs}) == [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8191, 8192] and len(refs) == 36
    for (ln, variant), g in refs.items():
        assert len(g) == ln
        want = {"clean": [], "n_last": [ln - 1], "n_last_two_and_first": sorted({0, max(0, ln - 2), ln - 1})}[variant]
        assert np.flatnonzero(g >= 4).tolist() == want, (ln, variant)
        assert pr.ends_windows(ln) == [(0, ln), (ln - min(ln, 70), min(ln, 70)), (ln - 1, 1)]
        assert len(pr.ends_reads(ln, variant)) == 3
    assert {ln % 16 for ln in pr.ENDS_LENGTHS} >= {0, 1, 15} and {ln % 4096 for ln in pr.ENDS_LENGTHS} >= {0, 1, 4095}


def test_window_classes():
    g = pr.main_ref()
    sm, em = pr.windows("start_mod"), pr.windows("end_mod")
    assert [s for s, _ in sm] == list(range(4040, 4104)) and {l for _, l in sm} == {300}
    assert {s for s, _ in em} == {3900} and [s + l for s, l in em] == list(range(4050, 4114))
    assert {s % 64 for s, _ in sm} == set(range(64)) and {(s + l) % 64 for s, l in em} == set(range(64))
    assert {s % 16 for s, _ in sm} == set(range(16)) and {(s + l - 1) % 64 for s, l in em} == set(range(64))
    # beside_n: the four windows of every stretch (three at either end of the reference)
    bn = set(pr.windows("beside_n")) | set(pr.windows("bad_bytes"))
    p, clean_and_dirty = pr.pack(g), 0
    for lo, hi in pr.stretches(g):
        b = pr.beside(g, lo, hi)
        assert set(b) == ({"after", "from"} if lo == 0 else {"before", "onto"} if hi == len(g) else {"before", "onto", "after", "from"}), (lo, hi)
        assert set(b.values()) <= bn
        for which, (s, l) in b.items():
            w = g[s:s + l]
            assert l >= 2 or which in ("before", "after")
            if which == "before":
                assert s + l == lo and (w < 4).all(), (lo, hi)
                assert pr.dirty(p, s, l) == ((lo - 1) >> 6 == lo >> 6), (lo, hi)  # dirty and clean, unless the stretch begins its block
                clean_and_dirty += pr.dirty(p, s, l)
            if which == "after":
                assert s == hi and (w < 4).all(), (lo, hi)
                assert pr.dirty(p, s, l) == (hi >> 6 == (hi - 1) >> 6), (lo, hi)  # ... or ends it
                clean_and_dirty += pr.dirty(p, s, l)
            if which == "onto":
                assert s + l == lo + 1 and np.flatnonzero(w >= 4).tolist() == [l - 1]
            if which == "from":
                assert s == hi - 1 and np.flatnonzero(w >= 4).tolist() == [0]
    assert len(pr.windows("beside_n")) == 4 * 70 - 2 - 2 - 2 and clean_and_dirty >= 130
    assert all((g[s:s + l] == 4).all() for s, l in pr.windows("all_n")) and {l for _, l in pr.windows("all_n")} == {1, 64, 150}
    fw = pr.windows("full_word")
    assert fw[0] == (8100, 4300) and len(fw) == 4 and all(8100 <= s and s + l <= 12400 for s, l in fw) and max(l for _, l in fw) == 4300
    te = pr.windows("to_the_end")
    assert [l for _, l in te] == [1, 16, 64, 65, 300] and all(s + l == pr.MAIN_LEN for s, l in te)
    ce = pr.windows("clean_edges")
    assert [pr.dirty(p, s, l) for s, l in ce] == [True] * 3 + [False] * 15 and all((g[s:s + l] < 4).all() for s, l in ce)
    for s, l in ce:  # a flagged block right before or right behind every one of them
        assert pr.dirty(p, s - 1, 1) or pr.dirty(p, s + l, 1) or pr.dirty(p, s, l), (s, l)
    assert {(s, l) for s, l in ce if s + l == 8192} and 8192 % 4096 == 0 and 20480 // 64 == (pr.MAIN_LEN - 1) // 64  # one past: flag word 2; the last block
    assert len({(s, l) for s, l in ce if s + l == 20480}) == 3 and len({(s, l) for s, l in ce if s == 12288}) == 3
    bad, ok = pr.windows("bad_bytes"), pr.windows("bad_bytes_ok")
    assert (0, pr.MAIN_LEN) in bad and all((g[s:s + l] >= 5).any() for s, l in bad) and len(bad) == 7
    assert ok[0][0] + ok[0][1] == 16000 and ok[1][0] == 16040 and all((g[s:s + l] < 5).all() for s, l in ok)
    eb = pr.windows("every_base")
    assert len(eb) == 20477 and {l for _, l in eb} == {1} and len({s for s, _ in eb}) == 20477 and not any(16000 <= s < 16040 for s, _ in eb)
    for name in pr.RUN_CLASSES:
        assert all(l >= 1 and 0 <= s and s + l <= pr.MAIN_LEN and (g[s:s + l] < 5).all() for s, l in pr.windows(name)), name
        assert all(l <= 4300 for _, l in pr.windows(name))


def test_reads_stay_related_and_the_certificate_takes_its_share():
    g = pr.main_ref()
    for blocks, (lo, hi) in ((1, (20, 150)), (2, (161, 330))):
        for name in pr.RUN_CLASSES:
            rs = pr.reads(name, blocks)
            assert len(rs) == len(pr.windows(name))
            assert all(r.dtype == np.uint8 and (r <= 4).all() and len(r) >= 1 for r in rs)
            exact = [r for k, r in enumerate(rs) if k % 3]
            assert all(lo <= len(r) <= hi for r in exact), name
    rs = pr.reads("start_mod")
    assert any((r == 4).any() for r in rs[2::3]) and not any((r == 4).any() for r in rs[1::3])  # the third kind keeps the window's N
    for k, (s, l) in enumerate(pr.windows("start_mod")):
        if k % 3 == 2:  # an exact copy lies in its window
            w, r = g[s:s + l].tobytes(), rs[k].tobytes()
            assert r in w
    assert max(len(r) for r in pr.reads("full_word", 2)) > 320 and min(len(r) for r in pr.reads("start_mod", 2)) > 160 and max(len(r) for n in pr.RUN_CLASSES for r in pr.reads(n)) <= 150
    admitted, refused = pr.certificate_counts()
    n = len(pr.windows("start_mod")) + len(pr.windows("beside_n"))
    assert admitted + refused == n and 4 * admitted >= n and refused >= 1


@pytest.mark.parametrize("which", ["main"] + ["ends_%d" % ln for ln in pr.ENDS_LENGTHS] + ["synthetic"])
def test_the_restated_layout_gives_back_the_bytes(which):
    if which == "main":
        refs = [pr.main_ref()]
    elif which == "synthetic":  # the host statement of the synthetic reference, where the read-back looks: the run behind the pass border
        from gonomics_amd import _lib
        pos = pr.syn_positions()
        assert pos[-1] == pr.SYN_LEN - 1 and pr.PASS in pos and pos.shape[0] == 3 * 141 + 570
        b = _lib.synthetic_reference_positions(pos, pr.SYN_SEED)
        assert (b[pos >= 300000000] == 4).all() and (b[(pos >= 250000000) & (pos < 250001000)] == 4).all()
        assert (b[(pos < 250000000) | ((pos >= 250001000) & (pos < 300000000))] < 4).all()
        first = (300000000 // 4096) * 4096
        refs = [_lib.synthetic_reference_bases(first, pr.SYN_LEN - first, pr.SYN_SEED)]  # from a flag-word border to the end
    else:
        ln = int(which.split("_")[1])
        refs = [pr.ends_refs()[(ln, v)] for v in pr.ENDS_VARIANTS]
    for g in refs:
        p = pr.pack(g)
        want = np.minimum(g, 5)
        assert p.words.shape[0] == (len(g) + 63) // 64 * 4 and p.flags.shape[0] == p.ranks.shape[0] == ((len(g) + 63) // 64 + 63) // 64
        assert p.masks.shape[0] == sum(bin(int(f)).count("1") for f in p.flags) == pr.flagged_blocks(g)
        assert np.array_equal(pr.values(p), want)
        step = max(1, len(g) // 997)
        for x in list(range(0, len(g), step)) + [len(g) - 1] + [x for lo, hi in pr.stretches(g)[:80] for x in (lo - 1, lo, hi - 1, hi) if 0 <= x < len(g)]:
            assert pr.value(p, x) == want[x], x
        assert not (p.masks[:, 0] & p.masks[:, 1]).any()


def test_dirty_is_a_flagged_block_under_the_window():
    g = pr.main_ref()
    p = pr.pack(g)
    blocks = (g[:20480].reshape(-1, 64) >= 4).any(axis=1).tolist() + [True]
    for name in pr.RUN_CLASSES + ("bad_bytes", "bad_bytes_ok"):
        for s, l in pr.windows(name):
            assert pr.dirty(p, s, l) == any(blocks[s >> 6:((s + l - 1) >> 6) + 1]), (name, s, l)
    assert pr.flagged_blocks(g) == sum(blocks)
