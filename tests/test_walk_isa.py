"""ISA of the random-walk kernels (csrc/kernels/walk.hip) in the shipped library, read with scripts/check_isa.py's helpers
(its rules untouched): every rwalk_* instantiation — the uniform kernel for the four (start dtype, col dtype) pairs, the
weighted one for those times (float, double) weights — uses no scratch and spills no VGPR (a lane keeps its walk's generator,
its current node and, in the weighted form, its best key in registers), and stays at or below 64 VGPRs, the budget of eight
waves per SIMD that the uniform kernel's latency hiding is planned on. The kernel names stay clear of the patterns the other
ISA tests count."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTED = (r"\bsample_\w*_kernel", r"\bagg\w*", r"\bgat_\w+", r"\bgatv2_\w+", r"\bgat_edge_\w+", r"\brelagg_", r"\baggw_",
           r"\bagg16_", r"\baggg_", r"\bqrows_", r"\btconv_", r"\bpna_")


def test_walk_kernels_without_scratch_or_spills(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from wholegraph_amd import binding
    seen, full = {}, []
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(r"\b(rwalk_\w+_kernel)<([^>]*)>\(", dn)
                if not m or "[clone" in dn or mangled not in meta:
                    continue
                full.append(dn)
                seen[m.group(1) + "<" + m.group(2) + ">"] = meta[mangled]
    ids = ("int", "long")
    want = {"rwalk_uniform_kernel<%s, %s>" % (a, b) for a in ids for b in ids}
    with open(os.path.join(ROOT, "wholegraph_amd", "csrc", "kernels", "walk.hip")) as f:
        group = int(re.search(r"constexpr int kWalkGroup = (\d+);", f.read()).group(1))     # lanes per weighted walk
    want |= {"rwalk_weighted_kernel<%s, %s, %s, %d>" % (a, b, w, group) for a in ids for b in ids for w in ("float", "double")}
    assert len(want) == 12 and set(seen) == want, sorted(want ^ set(seen))
    bad = {k: v[1:] for k, v in seen.items() if tuple(v[1:]) != (0, 0)}
    assert not bad, "(spilled VGPRs, scratch bytes): %s" % bad
    wide = {k: v[0] for k, v in seen.items() if v[0] > 64}
    assert not wide, "VGPRs above the eight-waves-per-SIMD budget: %s" % wide
    # the existing ISA tests count what these patterns find: none of the new kernels' names may be among it
    for dn in full:
        name = re.search(r"\brwalk_\w+_kernel", dn).group(0)
        for pattern in COUNTED:
            assert not re.search(pattern, name), (pattern, dn)
        # ... nor a rule of scripts/check_isa.py
        for rule, _ in ci.RULES + ci.EXCEPTIONS:
            assert not re.search(rule, dn), (rule, dn)
