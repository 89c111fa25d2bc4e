"""Registers and LDS of the gapless-certificate kernels (fp_cert.hip.h), read from the gfx950 code object like tests/test_kernel_resources.py
does (CPU suite).  The scan is a latency-bound stream -- one 16-byte load per lane and round -- so it lives on waves in flight: its
registers must allow the full eight waves per SIMD, its LDS (the read's k-mer table, the prefilter, four staged base rows) at least 20
one-wave workgroups per CU, and nothing may go to scratch."""
import os

import pytest

from test_kernel_resources import LLVM, _kernels, _waves_per_simd

CERT_KERNELS = ("fp_cert_kernel<false>", "fp_cert_kernel<true>", "fp_cert_gather_kernel")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    return _kernels(tmp_path_factory.mktemp("co_cert"))


def test_cert_kernels_are_in_the_library(kernels):
    for name in CERT_KERNELS:
        assert name in kernels, (name, [k for k in kernels if "cert" in k])


def test_cert_kernel_registers_and_scratch(kernels):
    for name in CERT_KERNELS:
        k = kernels[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["agpr_count"] == 0 and k["vgpr_count"] <= 64 and _waves_per_simd(k) == 8, (name, k)


def test_cert_kernel_lds_granules(kernels):
    # LDS is handed out in granules of 1280 B on gfx950 (160 KB per CU): 6 granules = 21 one-wave workgroups per CU
    for name in CERT_KERNELS[:2]:
        assert (kernels[name]["group_segment_fixed_size"] + 1279) // 1280 <= 6, (name, kernels[name]["group_segment_fixed_size"])
    assert kernels["fp_cert_gather_kernel"]["group_segment_fixed_size"] == 0
