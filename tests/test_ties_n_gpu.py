"""Tie-breaking in the kernels of the chunk / group DPs (N1) and of the graph aligner's seed-extension DPs (N2).  They apply
tripleMaxTrace's rule -- M over I over D -- in code of their own: fill_affine_kernel<.., SCORED> (rebased and plain tables),
lat_fill_kernel<.., SCORED, S16>, lat_wide_kernel<.., SCORED> behind an int16 or int32 score matrix of score_matrix_*_kernel, walked
by traceback_kernel (one lane per pair, one wave per pair in one pass and in two); fill_const_kernel<MULTI, GSW, P16> walked by
gsw_traceback_kernel.  tests/test_n1_gpu.py and tests/test_n2_gsw.py run them under penalties where two gaps never beat or equal
a cell score on a route, so a kernel that prefers D over I passes them.  Here every route -- forced with the switches those suites
use, asserted through the timing's fast_path where it tells routes apart -- runs tests/ties_n.py's sets on its batches and must
give the oracle's scores, offsets, runs, ops and (extensions) ends bit for bit.  Before each run ties_n.decisive_* holds (cached):
by the census of the reference's own route the wrong order of preference changes at least half of the pairs
(tests/test_ties_n_cpu.py shows it without a GPU).  DESIGN.md 4.33."""
import numpy as np
import pytest

import common
import n1_helpers
import oracle
import ties_n
from gonomics_amd import align, fasta

pytestmark = pytest.mark.gpu

SWITCHES = ("GNX_FASTPATH", "GNX_CLONG", "GNX_NO_HFORM", "GNX_LAT", "GNX_WIDE", "GNX_MEGA_STRIPS", "GNX_W64", "GNX_SCORED_SUB", "GNX_TB_TWO_PASS",
            "GNX_NO_PIPE", "GNX_CONST_P32", "GNX_SCORE_SWEEP", "GNX_N1_SCORE_FIRST")
LAT, GENERAL, PLAIN, WIDE = {"GNX_LAT": "2"}, {"GNX_LAT": "0"}, {"GNX_LAT": "0", "GNX_NO_HFORM": "1"}, {"GNX_WIDE": "2"}
ROUTE_OF = {"lat": (LAT, 3), "general": (GENERAL, 0), "plain": (PLAIN, 0), "wide": (WIDE, 4)}


@pytest.fixture(autouse=True)
def _own_switches(monkeypatch):
    """the routes are this module's to choose: every case starts without the switches (tools/switch_matrix.sh sets some from outside)"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _rows(sc, ops, off):
    return [(int(sc[k]), [(int(r), int(o)) for r, o in zip(ops["run_length"][off[k]:off[k + 1]], ops["op"][off[k]:off[k + 1]])]) for k in range(len(sc))]


def _n1(L, name, chunk, sname, route, what=""):
    """a named N1 batch under the switches in force: a case on which the ties decide, the oracle's bits, the route asked for"""
    assert ties_n.decisive_n1(name, chunk, sname)
    table, go, ge = ties_n.n1_params(sname)
    p = L.make_params(L.GNX_AFFINE_GAP_HIGHMEM, table, go, ge)
    if name == "g_small":
        blocks, pairs = ties_n.group_batch(chunk)
        got = L.multiple_affine_gap_batch(p, chunk, blocks, pairs)
    else:
        got = L.affine_gap_chunk_batch(p, chunk, *ties_n.chunk_batch(name, chunk))
    tm = L.get_timing()
    exp = ties_n.n1_expected(name, chunk, sname)
    bad = [(k, g, e) for k, (g, e) in enumerate(zip(_rows(*got), exp)) if g != e]
    assert not bad, ("%s chunk %d %s (%d, %d) %s: %d pairs differ" % (name, chunk, sname, go, ge, what, len(bad)), bad[0])
    if route is not None and not common.OUTER_ROUTE_SWITCH:
        assert tm["fast_path"] == route, (tm["fast_path"], route, name, chunk, sname, what)


# ---- N1: the chunk DP ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lat", "general", "plain", "wide"])
@pytest.mark.parametrize("chunk", ties_n.C_CHUNKS["c_small"])
def test_chunk_one_strip(gpu_lib, monkeypatch, chunk, route):
    """c_small, at most 160 chunk cells a side: lat_fill_kernel<.., SCORED> (the library's own choice for small calls),
    fill_affine_kernel<.., SCORED> on one strip with the rebased and with the plain tables, lat_wide_kernel<.., SCORED>; chunk
    1, 2, 3 (score_matrix_pairs_kernel<S16, CH>) and 5 (the generic score_matrix_kernel); at chunk 5 the scaled set runs the int32
    score matrix under the same ties"""
    env, fast_path = ROUTE_OF[route]
    _set(monkeypatch, env)
    for sname in ties_n.N1_PLAN[("c_small", chunk)]:
        _n1(gpu_lib, "c_small", chunk, sname, fast_path, route)


@pytest.mark.parametrize("chunk", ties_n.C_CHUNKS["c_small"])
def test_chunk_in_sub_batches(gpu_lib, monkeypatch, chunk):
    """GNX_SCORED_SUB=4: the batch in four sub-batches (run_host_scored), offsets of each shifted behind the one before"""
    _set(monkeypatch, dict(GENERAL, GNX_SCORED_SUB="4"))
    for sname in ties_n.N1_PLAN[("c_small", chunk)]:
        _n1(gpu_lib, "c_small", chunk, sname, 0, "four sub-batches")


@pytest.mark.parametrize("route", ["lat", "general", "general_two_pass", "general_no_pipe", "plain", "wide"])
@pytest.mark.parametrize("chunk", ties_n.C_CHUNKS["c_long"])
def test_chunk_several_strips(gpu_lib, monkeypatch, chunk, route):
    """c_long, 170 .. 450 x 200 .. 600 chunk cells: several strips in every pair, piped under GNX_LAT=0 (the longest beta has 512
    columns or more) and one launch per strip row under GNX_NO_PIPE; the walk by one wave per pair (the longest side is 256 or more)
    in one pass and, under GNX_TB_TWO_PASS, as count + write"""
    al, be = ties_n.chunk_batch("c_long", chunk)
    assert min(len(a) // chunk for a in al) > 160 and max(len(b) // chunk for b in be) >= 512 and (len(al) + 3) // 4 < 3072
    assert max(max(len(a), len(b)) // chunk for a, b in zip(al, be)) >= 256
    env, fast_path = ROUTE_OF[route.split("_")[0]]
    _set(monkeypatch, env)
    if route == "general_two_pass":
        monkeypatch.setenv("GNX_TB_TWO_PASS", "1")
    if route == "general_no_pipe":
        monkeypatch.setenv("GNX_NO_PIPE", "1")
    for sname in ties_n.N1_PLAN[("c_long", chunk)]:
        _n1(gpu_lib, "c_long", chunk, sname, fast_path, route)


# ---- N1: the group DP -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lat", "general", "plain", "wide"])
@pytest.mark.parametrize("chunk", ties_n.G_CHUNKS)
def test_groups(gpu_lib, monkeypatch, chunk, route):
    """g_small through gnx_multiple_affine_gap_batch: every ordered pair of 8 alignment blocks (column averages truncated toward
    zero, lower case, gaps; score_profiles_kernel + score_matrix_groups_kernel<S16, CH>), blocks of up to 200 cells: one and two
    strips; at chunk 2 the scaled set runs the int32 matrix"""
    env, fast_path = ROUTE_OF[route]
    _set(monkeypatch, env)
    for sname in ties_n.N1_PLAN[("g_small", chunk)]:
        _n1(gpu_lib, "g_small", chunk, sname, fast_path, route)


# ---- N1: the score-only entries and the progressive driver -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,chunk", list(ties_n.N1_PLAN))
def test_score_entries(gpu_lib, name, chunk):
    """gnx_affine_gap_chunk_score_batch / gnx_multiple_affine_gap_score_batch: the oracle's scores under the same sets, by the
    sweep of n1_sweep.hip.h (route 9) wherever rule SS admits the set -- the scaled set falls back to the twin's route"""
    for sname in ties_n.N1_PLAN[(name, chunk)]:
        assert ties_n.decisive_n1(name, chunk, sname)
        table, go, ge = ties_n.n1_params(sname)
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, table, go, ge)
        if name == "g_small":
            blocks, pairs = ties_n.group_batch(chunk)
            got = gpu_lib.multiple_affine_gap_score_batch(p, chunk, blocks, pairs)
        else:
            got = gpu_lib.affine_gap_chunk_score_batch(p, chunk, *ties_n.chunk_batch(name, chunk))
        route = gpu_lib.get_timing()["fast_path"]
        assert [int(x) for x in got] == [s for s, _ in ties_n.n1_expected(name, chunk, sname)], (name, chunk, sname)
        if not common.OUTER_ROUTE_SWITCH:
            assert (route == 9) == (not sname.endswith("x40")), (name, chunk, sname, route)


@pytest.mark.parametrize("score_first", [None, "1"])
def test_all_seq_affine_chunk(gpu_lib, tmp_path, monkeypatch, score_first):
    """align.AllSeqAffineChunk on six related records of 60 chunks of 2 under hc3010 (-30, -10): the progressive alignment with the
    oracle as its pairwise engine, byte for byte -- every pair aligned every round, and score first"""
    if score_first:
        monkeypatch.setenv("GNX_N1_SCORE_FIRST", score_first)
    table, go, ge = ties_n.n1_params("hc3010")
    rng = np.random.default_rng(9201)
    base = np.resize(rng.integers(0, 4, size=3), 120).astype(np.uint8)
    base[:40] = rng.integers(0, 4, size=40)
    records = []
    for k in range(6):
        s = ties_n._mutate_cells(rng, base, 2, 0.05, 0.24)
        records.append(fasta.Fasta("r%d" % k, np.concatenate([s, base])[:120]))
    got = align.AllSeqAffineChunk(records, table, go, ge, 2)
    exp = n1_helpers.all_seq_affine_oracle(records, table, go, ge, 2)
    fasta.Write(str(tmp_path / "got.fa"), got)
    fasta.Write(str(tmp_path / "exp.fa"), exp)
    assert open(str(tmp_path / "got.fa"), "rb").read() == open(str(tmp_path / "exp.fa"), "rb").read()
    # the pairwise calls of the first round sit on ties: (M, D, I) would have changed at least half of them
    changed = [ties_n.walk_scored(ties_n.chunk_matrix(table, 2, records[x].Seq, records[y].Seq), go, ge, 2, (ties_n.MID, ties_n.MDI))
               for x in range(6) for y in range(x + 1, 6)]
    assert 2 * sum(c[ties_n.MID][1] != c[ties_n.MDI][1] for c in changed) >= len(changed)


# ---- N2: the extension DPs -----------------------------------------------------------------------------------------------------------------
def _ext(L, name, side, sname, what=""):
    assert ties_n.cross_condition() if name == "x_cross" else ties_n.decisive_ext(name, side, sname)
    table, gap = ties_n.ext_params(sname)
    al, be = ties_n.ext_batch(name, side)
    s, ei, ej, ops, off = L.gsw_extend_batch(L.GNX_GSW_LEFT if side == 0 else L.GNX_GSW_RIGHT, table, gap, al, be)
    got = [(sc, route, int(ei[k]), int(ej[k])) for k, (sc, route) in enumerate(_rows(s, ops, off))]
    exp = ties_n.ext_expected(name, side, sname)
    bad = [(k, len(al[k]), len(be[k]), g[0], g[2:], e[0], e[2:]) for k, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, ("%s side %d %s %s: %d pairs differ" % (name, side, sname, what, len(bad)), bad[0])
    return got


def _launch_shape(name, side):
    """(some pair has several 160-row strips, the longest read, groups of four pairs): what selects fill_const_kernel's launch"""
    al, be = ties_n.ext_batch(name, side)
    return max(len(a) for a in al) > ties_n.STRIP, max(len(b) for b in be), (len(al) + 3) // 4


@pytest.mark.parametrize("sname", list(ties_n.EXT_SETS))
@pytest.mark.parametrize("side", [0, 1])
def test_ext_one_strip(gpu_lib, side, sname):
    """x_small: fill_const_kernel<false, GSW, false> + gsw_traceback_kernel"""
    assert _launch_shape("x_small", side)[0] is False
    _ext(gpu_lib, "x_small", side, sname)


@pytest.mark.parametrize("sname", list(ties_n.EXT_SETS))
@pytest.mark.parametrize("side", [0, 1])
def test_ext_several_strips(gpu_lib, side, sname):
    """x_multi: several strips, reads below 512 columns: one launch, the strips of a group in turn (not piped).  The left walk
    rebuilds cell values from the final one, through tied cells, across strips"""
    multi, m_max, groups = _launch_shape("x_multi", side)
    assert multi and m_max < 512
    _ext(gpu_lib, "x_multi", side, sname)


@pytest.mark.parametrize("launch", ["piped_p16", "piped_p32", "no_pipe"])
@pytest.mark.parametrize("sname", list(ties_n.EXT_SETS))
@pytest.mark.parametrize("side", [0, 1])
def test_ext_piped(gpu_lib, monkeypatch, side, sname, launch):
    """x_piped: several strips, reads of 512 columns or more, fewer than 3 072 groups: the piped launch with the int16 profile
    (4 s + 3 fits for every set), with the int32 profile (GNX_CONST_P32), and strip after strip (GNX_NO_PIPE)"""
    multi, m_max, groups = _launch_shape("x_piped", side)
    assert multi and m_max >= 512 and groups < 3072
    table, _ = ties_n.ext_params(sname)
    assert all(-32768 <= 4 * v + 3 <= 32767 for row in table for v in row)
    if launch == "piped_p32":
        monkeypatch.setenv("GNX_CONST_P32", "1")
    if launch == "no_pipe":
        monkeypatch.setenv("GNX_NO_PIPE", "1")
    _ext(gpu_lib, "x_piped", side, sname, launch)


@pytest.mark.parametrize("launch", ["piped_p16", "piped_p32", "no_pipe"])
def test_ext_right_first_maximum_across_strips(gpu_lib, monkeypatch, launch):
    """the constructed pairs under the tie table and gap -15, reads of 520 columns or more: the maximum 10 p at (p, p) and again at
    (p + 4q, p + 4q), in strips 0 and 1, both in strip 2, in strips 1 and 2 (ties_n.cross_condition, on the CPU).  RightDynamicAln
    keeps the first; LeftDynamicAln on the same pairs for the walk"""
    multi, m_max, groups = _launch_shape("x_cross", 1)
    assert multi and m_max >= 512 and groups < 3072
    if launch == "piped_p32":
        monkeypatch.setenv("GNX_CONST_P32", "1")
    if launch == "no_pipe":
        monkeypatch.setenv("GNX_NO_PIPE", "1")
    got = _ext(gpu_lib, "x_cross", 1, "tie15", launch)
    assert [(g[0], g[2], g[3]) for g in got] == [(10 * p, p, p) for p, _ in ties_n.CROSS]
    _ext(gpu_lib, "x_cross", 0, "tie15", launch)
