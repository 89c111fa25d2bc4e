"""Registers, scratch and LDS of the four-wave form of the headline sweep (fp_sweep_kernel<RR, XP, PK, 4>), read from the
gfx950 code object like tests/test_kernel_resources.py does (CPU suite).  A workgroup of the four-wave form puts one wave on each SIMD of
its CU and three workgroups share a CU: its registers must allow three waves per SIMD, and its LDS -- one score table of 32 dwords and four
waves' profiles and base rings of 3344 dwords each: 53 632 B = 42 granules of 1280 B, three workgroups = 126 of a CU's 128 -- is sized at
launch, so the kernel itself declares none (the static budget of 11 granules that tests/test_kernel_resources.py pins for every
fp_sweep_kernel is the one-wave form's, and the real budget is pinned here)."""
import os
import re

import pytest

from test_kernel_resources import LLVM, ROOT, _kernels, _waves_per_simd

PARAMS = [(rr, xp, pk) for rr in (19, 20) for xp in ("false", "true") for pk in ("false", "true")]
FP8_LDS_BYTES = 4 * (32 + 3200 + 144)  # one wave's score table, profile and base rings (fp_sweep.hip.h: FP8_LDS dwords): 13 504 B
WG4_LDS_BYTES = 4 * (32 + 4 * (3200 + 144))  # the four-wave workgroup keeps the score table once: 53 632 B


def name(rr, xp, pk, wg):
    return "fp_sweep_kernel<%d, %s, %s, %d>" % (rr, xp, pk, wg)


def one_wave(rr, xp, pk):
    """the one-wave kernel of the same parameters (the transposed sweep of the packed reference has no one-wave form: nothing calls
    it -- its four-wave form is held to the transposed sweep of byte windows)"""
    return name(rr, xp, "false" if xp == "true" else pk, 1)


ONE_WAVE = sorted({(rr, xp, "false" if xp == "true" else pk) for rr, xp, pk in PARAMS})


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    return _kernels(tmp_path_factory.mktemp("co_wg4"))


def test_the_eight_four_wave_instantiations_exist(kernels):
    for rr, xp, pk in PARAMS:
        assert name(rr, xp, pk, 4) in kernels, (name(rr, xp, pk, 4), sorted(k for k in kernels if k.startswith("fp_sweep_kernel")))
    assert len([k for k in kernels if re.fullmatch(r"fp_sweep_kernel<\d+, \w+, \w+, 4>", k)]) == 8


def test_four_wave_registers_allow_three_waves_per_simd(kernels):
    for rr, xp, pk in PARAMS:
        k = kernels[name(rr, xp, pk, 4)]
        assert k["vgpr_count"] + k["agpr_count"] <= 168 and _waves_per_simd(k) >= 3, (name(rr, xp, pk, 4), k)


def test_four_wave_scratch_is_no_more_than_the_one_wave_kernel_has(kernels):
    for rr, xp, pk in PARAMS:
        k4, k1 = kernels[name(rr, xp, pk, 4)], kernels[one_wave(rr, xp, pk)]
        assert k4["private_segment_fixed_size"] <= k1["private_segment_fixed_size"], (name(rr, xp, pk, 4), k4, k1)


def test_four_wave_lds_is_sized_at_launch(kernels):
    """no static LDS; what the launch passes is 42 granules, so that three workgroups fit a CU's 128 (four whole one-wave images, 54 016 B,
    would be 43 granules: two workgroups per CU)"""
    for rr, xp, pk in PARAMS:
        assert kernels[name(rr, xp, pk, 4)]["group_segment_fixed_size"] == 0, name(rr, xp, pk, 4)
    assert (WG4_LDS_BYTES + 1279) // 1280 == 42 and 3 * 42 <= 128 < 3 * ((4 * FP8_LDS_BYTES + 1279) // 1280)
    src = open(os.path.join(ROOT, "gonomics_amd", "csrc", "fp_sweep.hip.h")).read()
    assert "FP_WG4_LDS_BYTES = (32 + FP_WG4 * FP8_SLICE) * 4" in src and "static_assert(FP_WG4_LDS_BYTES <= 42 * 1280" in src


def test_one_wave_forms_keep_the_parents_budgets(kernels):
    """the one-wave kernels are what they were: 13 504 B of static LDS (11 granules), three waves per SIMD by registers, the sweep's few
    bytes of prologue scratch at the most"""
    assert len(ONE_WAVE) == 6
    for rr, xp, pk in ONE_WAVE:
        k = kernels[name(rr, xp, pk, 1)]
        assert k["group_segment_fixed_size"] == FP8_LDS_BYTES and (k["group_segment_fixed_size"] + 1279) // 1280 == 11, (name(rr, xp, pk, 1), k)
        assert k["vgpr_count"] + k["agpr_count"] <= 168 and _waves_per_simd(k) == 3, (name(rr, xp, pk, 1), k)
        assert k["private_segment_fixed_size"] <= 256, (name(rr, xp, pk, 1), k)
