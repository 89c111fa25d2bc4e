"""The gapless certificate's decision the way fp_cert_kernel evaluates it -- 64 lanes with a chunk of consecutive rows each, wave sums and
scans -- restated on the host from the shared pieces of fp_cert_decide.h and held against gnx_cert_decide."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_decision_equals_the_serial_one(tmp_path):
    """tests/cpp/cert_wave_test.cpp: a host program with its own main, built with the address and undefined-behaviour sanitizers and
    run directly -- every n from 16 to 160, K from 1 to beyond n, buffers of exactly n and m bytes, the deficit's and the edge rule's
    boundaries, F_alpha > 0 first at a chunk's first and last row, ties for d*, d* = 0 / n - 1 / n, N and bytes >= 5, a refused matrix"""
    exe = str(tmp_path / "cert_wave_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "cert_wave_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
