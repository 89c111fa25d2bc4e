"""The sub-batch cut shared by the host flows (gonomics_amd/csrc/host_cut.h) is plain C++: tests/cpp/host_cut_test.cpp checks it on
the CPU -- whole waves, nothing past n, no empty sub-batch, equal to a restatement of the lines it replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "host_cut_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "host_cut_test.bin")


def test_host_cut():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "gonomics_amd", "csrc"), "-o", BIN, SRC])
    out = subprocess.run([BIN], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout
