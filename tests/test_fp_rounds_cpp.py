"""The launch plan of the four-wave headline sweep (gonomics_amd/csrc/fp_rounds.h) alone on the host (CPU suite)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_stand_alone(tmp_path):
    """tests/cpp/fp_rounds_test.cpp: a host program with its own main, built with the address and undefined-behaviour sanitizers --
    every pair count from 0 to past four rounds on 1, 2 and 256 CUs, rounds of 1, 2, 3 and 768 workgroups and the device's own"""
    exe = str(tmp_path / "fp_rounds_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "fp_rounds_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
