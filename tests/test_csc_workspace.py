"""csrc/csc_workspace.hpp — how the ops of a sampled CSC block lay out a device workspace (one function for the size to
allocate and for the offsets of the regions) — checked by brute force on the host: tests/cpp/csc_workspace_test.cpp
includes that header alone, is built here with the address and undefined-behaviour sanitizers of the host compiler and run
as a process of its own. No GPU, no library of the project, nothing loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_workspace_regions_are_aligned_disjoint_and_inside(tmp_path):
    exe = str(tmp_path / "csc_workspace_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "csc_workspace_test.cpp"), "-o", exe],
                        capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    p = subprocess.run([exe], capture_output=True, timeout=120)
    out = p.stdout.decode() + p.stderr.decode()
    assert p.returncode == 0 and "cases hold" in out, out[-4000:]
