"""tests/cpp/cert_edge_test.cpp: the graded edge rule's pieces of fp_cert_decide.h the way the kernel composes them -- 64 emulated lanes
with chunks of 1, 2 and 3 rows, non-free rows on both sides of the lane borders and on rows 0 and n - 1, as many grades as item 5 admits --
against the serial gnx_certe_decide.  A host program with its own main, built with the address and undefined-behaviour sanitizers and run
directly.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_pieces_against_the_serial_decision(tmp_path):
    exe = str(tmp_path / "cert_edge_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "cert_edge_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
