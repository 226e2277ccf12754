"""ISA of the small-fan-out weighted sampling kernel (csrc/kernels/graph.hip) in the shipped library, read with the helpers of
scripts/check_isa.py: every instantiation present, no scratch, no spilled VGPRs."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weighted_small_kernel_has_no_scratch_and_no_spills(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from wholegraph_amd import binding
    # no name-pattern rule of the row-kernel gate claims the new kernel
    assert not [pat for pat, _ in ci.RULES if re.search(pat, "sample_weighted_small_kernel<int, int, float, 32>")]
    seen = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(meta))
            for mangled, (vgprs, spilled, scratch) in meta.items():
                m = re.search(r"sample_weighted_small_kernel<(int|long), (int|long), (float|double), (32|64)>", names.get(mangled, ""))
                if m:
                    seen[m.groups()] = (vgprs, spilled, scratch)
    want = {(i, c, w, g) for i in ("int", "long") for c in ("int", "long") for w in ("float", "double") for g in ("32", "64")}
    assert set(seen) == want, sorted(want - set(seen))
    bad = {k: v for k, v in seen.items() if v[1] != 0 or v[2] != 0}
    assert not bad, "(VGPRs, spilled VGPRs, scratch bytes): %s" % bad
