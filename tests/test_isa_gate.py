"""Build-time gates on the shipped code (no GPU needed).

* scripts/check_isa.py: the gfx950 code object inside wholegraph_amd/libwholegraph.so is disassembled and the row kernels
  (gather / scatter / convert / flat / staged) and the gradient-apply tile kernel must show their batch of loads issued
  back to back (no s_waitcnt vmcnt between them), a VALU budget per tile, no register-shuffling share, no scratch.
  Round 3 shipped kernels whose SOURCE said "all loads of a batch are issued before its first store" while the ISA waited
  for every load: this is the check that reads the ISA.
* every environment knob of the library goes through WM_KNOB (read once, wholememory_ext_reload_knobs re-reads): no
  getenv call is left on any op's path."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shipped_kernels_keep_their_loads_in_flight(wm_lib):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_isa.py")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "all rules hold" in p.stdout
    # the headline kernel is among the checked ones
    assert re.search(r"rows_batch_kernel<long, true, 32, false, 0>.*\bok\b", p.stdout)
    assert re.search(r"step_tile_kernel<long, 1, 2, false, float, 16, false>.*\bok\b", p.stdout)
    # ... and the 8-byte-piece instantiation of round 6 (fp32 rows of whole 8-byte pieces: 602 floats)
    assert re.search(r"step_tile_kernel<long, 1, 1, false, float, 8, false>.*\bok\b", p.stdout)
    # ... and the ragged one (rows of dim % 4 != 0 floats: the reference's own test dims 513 / 129 / 127)
    assert re.search(r"step_tile_kernel<long, 1, 1, false, float, 16, true>.*\bok\b", p.stdout)


def test_no_getenv_outside_the_knob_reader():
    offenders = []
    for f in glob.glob(os.path.join(ROOT, "wholegraph_amd", "csrc", "**", "*"), recursive=True):
        if not f.endswith((".cpp", ".hpp", ".hip", ".cuh")) or f.endswith("knobs.hpp"):
            continue
        for n, line in enumerate(open(f), 1):
            code = line.split("//")[0]
            if re.search(r"(?<![A-Za-z_])(std::)?getenv\s*\(", code):
                offenders.append("%s:%d: %s" % (os.path.relpath(f, ROOT), n, line.strip()))
    assert not offenders, "getenv outside knobs.hpp (use WM_KNOB):\n" + "\n".join(offenders)


def test_reload_knobs_is_exported(wm_lib):
    from wholegraph_amd import binding
    binding.reload_knobs()
