"""csrc/exchange_plan.hpp — the index arithmetic of the chunked row exchange that the distributed gather, the distributed
scatter and the sparse gradient apply are built on — checked by brute force on the host: tests/cpp/exchange_plan_test.cpp
includes that header alone, is built here with the address and undefined-behaviour sanitizers of the host compiler and run
as a process of its own. No GPU, no library of the project, nothing loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exchange_plan_holds_on_the_grid(tmp_path):
    exe = str(tmp_path / "exchange_plan_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "exchange_plan_test.cpp"), "-o", exe],
                        capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    p = subprocess.run([exe], capture_output=True, timeout=120)
    out = p.stdout.decode() + p.stderr.decode()
    assert p.returncode == 0 and "cases hold" in out, out[-4000:]
