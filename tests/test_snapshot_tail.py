"""The end of a device call on the snapshot path (run_device_clong, run_device_mega: routes 2, 6 and 5 of gnx_timing.fast_path): the error
flags and the CIGAR run count read back from the device, reported as the drivers of every route report them -- a base >= 5 is GNX_EBASE with
its message, a CIGAR buffer that was guessed too small is grown by the host flow and the sub-batch runs again."""
import numpy as np
import pytest

import common
import oracle
from test_host_entry import _first_sub_batch_that_grows, _many_runs_case
from test_long_range import _related

pytestmark = pytest.mark.gpu
MX = common.matrices()

ROUTES = {2: {"GNX_CLONG": "2", "GNX_W64": "0"},  # the 16-lane sweeps and walks
          6: {"GNX_CLONG": "2", "GNX_W64": "2"},  # the whole wave on one pair, the walk farm
          5: {"GNX_MEGA_STRIPS": "2"}}            # row panels of two strips


@pytest.mark.parametrize("route", [2, 6, 5])
@pytest.mark.parametrize("mode", [0, 1])
def test_bad_base_through_each_snapshot_route(gpu_lib, monkeypatch, mode, route):
    """one byte 5 in the last pair's alpha: the call is GNX_EBASE with the message of every route; without it the same call equals the oracle"""
    for k in ("GNX_CLONG", "GNX_W64", "GNX_MEGA_STRIPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(90 + mode)
    a0, b0 = _related(rng, 700, 200, sub=0.05, indel=0.03)
    a1 = rng.integers(0, 4, size=1500).astype(np.uint8)
    b1 = common.mutate(rng, a1[500:900], sub=0.05, indel=0.03, geo=0.4)
    a2, b2 = _related(rng, 300, 1700, sub=0.05, indel=0.03)
    alphas, betas = [a0, a1, a2], [b0, b1, b2]
    name, go, ge = ("HumanChimpTwo", -600, -150) if mode == 0 else ("HumanChimpTwo", -430, 0)
    p = gpu_lib.make_params(mode, MX[name], go, ge)
    got = gpu_lib.align_batch(p, alphas, betas)
    assert gpu_lib.get_timing()["fast_path"] == route
    common.assert_same(got, oracle.align_batch(mode, MX[name], go, ge, alphas, betas, threads=4), "mode %d route %d" % (mode, route))
    bad = a2.copy()
    bad[137] = 5
    with pytest.raises(gpu_lib.GnxError) as ei:
        gpu_lib.align_batch(p, [a0, a1, bad], betas)
    assert ei.value.code == gpu_lib.GNX_EBASE
    assert "a base >= 5 was found: the reference would panic (index out of range)" in str(ei.value)


def test_cigar_capacity_growth_through_route_2(gpu_lib, monkeypatch):
    """tests/test_host_entry.py's many-runs batch through run_device_clong: the first guess of 2^20 runs overflows, the driver reports
    GNX_ECAPACITY with the count it needs, the host flow grows the buffer and runs the sub-batch again (routes 5 and 6 end in the same
    tail; 2 048 one-pair panel runs would take too long)"""
    n = 2048
    mx, a, b, starts, lens, per, exp = _many_runs_case(n)
    # preconditions, from the oracle alone: the one sub-batch of the call exceeds the first guess
    assert n * per > 1 << 20
    assert _first_sub_batch_that_grows(n, 131072, per) == (0, 0)
    monkeypatch.delenv("GNX_HOST_SUB", raising=False)
    monkeypatch.delenv("GNX_MEGA_STRIPS", raising=False)
    monkeypatch.setenv("GNX_CLONG", "2")
    monkeypatch.setenv("GNX_W64", "0")
    p = gpu_lib.make_params(gpu_lib.GNX_CONST_GAP, mx, 0)
    common.assert_same(gpu_lib.align_batch_windows(p, a, starts, lens, b, starts, lens), exp, "route 2, grown once")
    assert gpu_lib.get_timing()["fast_path"] == 2
