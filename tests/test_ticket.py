"""Forward progress of the pipelined launches must not depend on the order in which workgroups start (VERDICT r2 item 3;
MI355X_MICROARCH "Workgroup dispatch": HIP promises nothing about dispatch order).  In every piped kernel a workgroup CLAIMS its item
and every unclaimed predecessor of it, and runs those first (csrc/gnx_common.hip.h: claim_items): nobody waits for work that has not been
taken.  Two stress legs, each over all piped kernels, results against the oracle:
  * GNX_TICKET_DELAY: the workgroups of the lower half of the grid sleep before they claim, so the upper half finds its predecessors
    unclaimed and runs whole chains itself (what a dispatcher that starts workgroups in another order would cause);
  * gnx_debug_occupy: 128 workgroups that each hold a whole CU's LDS spin on another stream while the piped launch runs, so half
    the CUs cannot take workgroups of the launch at all.
  * steal: the delay alone never makes anybody TAKE an item -- the default grace period (20 ms) outlasts it.  This leg
    sets GNX_CLAIM_GRACE_US=50 for the launch together with a delay of ~2 ms, so the upper half of the grid really claims and runs its
    predecessors' items (the s_lo .. s_own loops of the strip kernels, the level loop of fp_sweep_levels_kernel), and asserts through
    gnx_debug_counter(0) that at least one item was run by a workgroup other than its own.
The three levels kernels of the score-only sweeps (score_sweep.hip.h, n1_sweep.hip.h) share one workgroup loop and are not reached
by align_batch: test_score_levels_do_not_depend_on_dispatch_order drives them through their own entries, delay and steal legs.
The bug trap (5 s spin timeout -> error flag 16 -> sequential re-run) must stay silent: the legs assert that the piped launch was
the one that produced the result by checking that the call took far less than the timeout."""
import functools
import os
import time

import numpy as np
import pytest

import common
import oracle

pytestmark = pytest.mark.gpu
MX = common.matrices()


def _pairs(seed, n_pairs, n_lo, n_hi, m_lo, m_hi):
    rng = np.random.default_rng(seed)
    alphas, betas = [], []
    for _ in range(n_pairs):
        m = int(rng.integers(m_lo, m_hi + 1))
        b = rng.integers(0, 4, size=m).astype(np.uint8)
        n = int(rng.integers(n_lo, n_hi + 1))
        o = int(rng.integers(0, max(1, m - n)))
        a = common.mutate(rng, b[o:o + n], sub=0.05, indel=0.02, geo=0.4, alphabet=4)
        if len(a) == 0:
            a = b[:1].copy()
        alphas.append(a); betas.append(b)
    return alphas, betas


# (name, environment that routes the batch to the kernel, mode, matrix, penalties, pairs)
LEGS = [
    ("fill_affine_kernel<MULTI> piped strips", {"GNX_FASTPATH": "0", "GNX_LAT": "0"}, 0, "HumanChimpTwo", (-600, -150), (101, 6, 900, 1400, 2200, 2600)),
    ("fill_const_kernel<MULTI> piped strips", {"GNX_CLONG": "0", "GNX_LAT": "0"}, 1, "Default", (-430, 0), (102, 6, 900, 1400, 2200, 2600)),
    ("cl_sweep_wg_kernel piped items of 5 strips", {"GNX_CLONG": "2", "GNX_W64": "0"}, 1, "HumanChimpTwo", (-430, 0), (103, 6, 1700, 2500, 2200, 2600)),
    ("cl_sweep_kernel piped strips", {"GNX_CLONG": "2", "GNX_CL_WG": "0", "GNX_W64": "0"}, 1, "HumanChimpTwo", (-430, 0), (103, 6, 900, 1400, 2200, 2600)),
    ("al_sweep_kernel piped strips", {"GNX_CLONG": "2", "GNX_FASTPATH": "0", "GNX_W64": "0"}, 0, "HumanChimpTwo", (-600, -150), (104, 6, 900, 1400, 2200, 2600)),
    ("fp_sweep_levels_kernel (row blocks)", {"GNX_FASTPATH": "2"}, 0, "HumanChimpTwo", (-600, -150), (105, 96, 500, 800, 1500, 1800)),
    # round 5: the latency geometry's strips (one wave per strip, rows handed over through sentinel-marked memory) and its int64 form
    ("lat_fill_kernel<affine> piped strips", {"GNX_LAT": "2"}, 0, "HumanChimpTwo", (-600, -150), (106, 6, 900, 1400, 2200, 2600)),
    ("lat_fill_kernel<const> piped strips", {"GNX_LAT": "2"}, 1, "Default", (-430, 0), (107, 6, 900, 1400, 2200, 2600)),
    ("lat_wide_kernel piped strips", {"GNX_WIDE": "2"}, 0, "HumanChimpTwo", (-600, -150), (108, 6, 900, 1400, 2200, 2600)),
    # the snapshot path with the whole wave on one pair (strips of 640 rows)
    ("al64_sweep_kernel piped strips", {"GNX_CLONG": "2", "GNX_FASTPATH": "0", "GNX_W64": "2"}, 0, "HumanChimpTwo", (-600, -150), (109, 5, 2000, 3800, 3000, 4200)),
    ("cl64_sweep_kernel piped strips", {"GNX_CLONG": "2", "GNX_W64": "2"}, 1, "HumanChimpTwo", (-430, 0), (110, 5, 2000, 3800, 3000, 4200)),
]


@pytest.mark.parametrize("leg", LEGS, ids=[x[0].split()[0].replace("<", "_").replace(">", "") for x in LEGS])
@pytest.mark.parametrize("stress", ["delay", "occupy", "both", "steal"])
def test_piped_launches_do_not_depend_on_dispatch_order(gpu_lib, monkeypatch, leg, stress):
    name, env, mode, mx, (go, ge), spec = leg
    alphas, betas = _pairs(*spec)
    exp = oracle.align_batch(mode, MX[mx], go, ge, alphas, betas, 10000, 10000, threads=8)
    p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP if mode == 0 else gpu_lib.GNX_CONST_GAP, MX[mx], go, ge)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")
    plain = gpu_lib.align_batch(p, alphas, betas)
    common.assert_same(plain, exp, name)
    gpu_lib.debug_counter(0, reset=True)
    if stress == "steal":
        monkeypatch.setenv("GNX_TICKET_DELAY", "600")     # ~ 600 x 127 x 64 cycles = 2 ms before the lower half claims ...
        monkeypatch.setenv("GNX_CLAIM_GRACE_US", "50")    # ... and a successor takes an unclaimed predecessor after 50 us
    if stress in ("delay", "both"):
        monkeypatch.setenv("GNX_TICKET_DELAY", "40")   # ~ 40 x 127 x 64 cycles = 0.15 ms before the lower half claims
    if stress in ("occupy", "both"):
        gpu_lib.check(gpu_lib.lib().gnx_debug_occupy(128, 300))  # half the CUs gone for 0.3 s
    t0 = time.time()
    got = gpu_lib.align_batch(p, alphas, betas)
    dt = time.time() - t0
    common.assert_same(got, exp, name + " / " + stress)
    assert dt < 3.0, "%s: %.1f s -- the spin timeout fired, the pipeline did not make progress on its own" % (name, dt)
    stolen = gpu_lib.debug_counter(0, reset=True)
    if stress == "steal" and not common.OUTER_ROUTE_SWITCH and "GNX_NO_PIPE" not in os.environ:
        assert stolen > 0, "%s: nobody ran a predecessor's item -- the n_stolen > 0 paths were not exercised" % name
    time.sleep(0.35)  # let the occupying workgroups end before the next test


# ---- the score-only sweeps: score_sweep_levels_kernel<true>, score_local_levels_kernel, n1_sweep_levels_kernel ------------------------
@functools.lru_cache(maxsize=None)
def _score_levels_case():
    """16 pairs = four quads of two and three row blocks, one quad of both (the side held in lanes: 161 .. 480 rows, one pair with
    exactly 161 = one real row in its top block; 300 .. 500 columns = several publishes of 64), and what the oracle says of them."""
    from test_locate_gpu import _ends
    rng = np.random.default_rng(111)
    n_rows = [161] + [int(x) for x in rng.integers(162, 321, size=6)] + [int(x) for x in rng.integers(321, 481, size=9)]
    rows, cols = [], []
    for n in n_rows:
        m = int(rng.integers(max(n, 300), 501))
        b = rng.integers(0, 4, size=m).astype(np.uint8)
        a = common.mutate(rng, b[:n], sub=0.05, indel=0.02, geo=0.4, alphabet=4)
        a = np.concatenate([a, rng.integers(0, 4, size=n).astype(np.uint8)])[:n]
        rows.append(a); cols.append(b)
    mx, go, ge = MX["HumanChimpTwo"], -600, -150
    exp_global = oracle.align_batch(0, mx, go, ge, rows, cols, threads=8)[0]
    sc, ops, off = oracle.align_batch(3, mx, go, ge, cols, rows, threads=8)
    exp_chunk = np.asarray([oracle.affine_gap_chunk(mx, go, ge, 1, a, b)[0] for a, b in zip(rows, cols)], dtype=np.int64)
    return rows, cols, {"global": (exp_global,), "local": (sc, _ends(ops, off, [len(t) for t in cols])), "chunk": (exp_chunk,)}


@pytest.mark.parametrize("route", ["global", "local", "chunk"])
@pytest.mark.parametrize("stress", ["delay", "steal"])
def test_score_levels_do_not_depend_on_dispatch_order(gpu_lib, monkeypatch, route, stress):
    rows, cols, expected = _score_levels_case()
    exp = expected[route]
    mx, go, ge = MX["HumanChimpTwo"], -600, -150
    if route == "global":    # global affine score: the shorter sequence is held in lanes
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP, mx, go, ge)
        call, fast_path = (lambda: (gpu_lib.score_batch(p, rows, cols),)), 7
    elif route == "local":   # local score and target end: the query is held in lanes
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_LOCAL, mx, go, ge)
        call, fast_path = (lambda: gpu_lib.locate_batch(p, cols, rows)), 8
    else:                    # chunk score with chunk 1: cell scores from a device matrix
        p = gpu_lib.make_params(gpu_lib.GNX_AFFINE_GAP_HIGHMEM, mx, go, ge)
        call, fast_path = (lambda: (gpu_lib.affine_gap_chunk_score_batch(p, 1, rows, cols),)), 9

    def same(got, what):
        assert len(got) == len(exp), what
        for g, e in zip(got, exp):
            assert np.array_equal(np.asarray(g, dtype=np.int64), e), (what, np.flatnonzero(np.asarray(g) != e)[:8])

    monkeypatch.setenv("GNX_DEBUG_ENTRY", "1")
    same(call(), route)
    routed = not common.OUTER_ROUTE_SWITCH and "GNX_SCORE_SWEEP" not in os.environ
    if routed:
        assert gpu_lib.get_timing()["fast_path"] == fast_path, (route, gpu_lib.get_timing())
    gpu_lib.debug_counter(0, reset=True)
    if stress == "steal":
        monkeypatch.setenv("GNX_TICKET_DELAY", "600")
        monkeypatch.setenv("GNX_CLAIM_GRACE_US", "50")
    else:
        monkeypatch.setenv("GNX_TICKET_DELAY", "40")
    t0 = time.time()
    got = call()
    dt = time.time() - t0
    same(got, route + " / " + stress)
    assert dt < 3.0, "%s: %.1f s -- the spin timeout fired, the pipeline did not make progress on its own" % (route, dt)
    stolen = gpu_lib.debug_counter(0, reset=True)
    if stress == "steal" and routed and "GNX_NO_PIPE" not in os.environ:
        assert stolen > 0, "%s: nobody ran a predecessor's item -- the n_stolen > 0 paths were not exercised" % route
