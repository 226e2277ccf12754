"""ISA of the temporal-sampler kernels (csrc/kernels/tsample.hip) in the shipped library, read with scripts/check_isa.py's
helpers (its rules untouched): exactly the expected tsample_* kernels exist — the count for the two centre dtypes at 16 lanes
per centre, the one-wave sum of the count's partial totals, and the select for the four (centre dtype, col dtype)
pairs at its two group sizes — they use no scratch, spill no VGPR and stay at or below 128 VGPRs. The kernel names stay clear
of the patterns the other ISA tests count. Only names and kernel metadata are looked at, as in tests/test_isub_isa.py."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tsample_kernels_without_scratch_or_spills(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from test_walk_isa import COUNTED
    from wholegraph_amd import binding
    seen, full = {}, []
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(r"\b(tsample_\w+)(?:<([^>]*)>)?\(", dn)
                if not m or "[clone" in dn or mangled not in meta:
                    continue
                full.append(dn)
                seen[m.group(1) + ("<" + m.group(2) + ">" if m.group(2) is not None else "")] = meta[mangled]
    ids = ("int", "long")
    want = {"tsample_count_kernel<%s, 16>" % a for a in ids} | {"tsample_total_kernel"}       # 16 lanes per centre in the count
    want |= {"tsample_select_kernel<%s, %s, %d>" % (a, b, g) for a in ids for b in ids for g in (32, 64)}
    assert len(want) == 11 and set(seen) == want, sorted(want ^ set(seen))
    print("VGPRs: %s" % {k: v[0] for k, v in sorted(seen.items())})
    bad = {k: v[1:] for k, v in seen.items() if tuple(v[1:]) != (0, 0)}
    assert not bad, "(spilled VGPRs, scratch bytes): %s" % bad
    wide = {k: v[0] for k, v in seen.items() if v[0] > 128}
    assert not wide, "VGPRs above the four-waves-per-SIMD budget: %s" % wide
    for dn in full:
        name = re.search(r"\btsample_\w+", dn).group(0)
        assert not re.search(r"rwalk_\w+_kernel", name) and not re.search(r"\bn2v_\w+", name), dn   # the walks' ISA tests
        assert not re.search(r"\bneg_\w+", name) and not re.search(r"\bedot_\w+", name), dn          # ... the later ones
        assert not re.search(r"\bisub_\w+", name), dn
        for pattern in COUNTED:                                  # ... and what the other ISA tests count
            assert not re.search(pattern, name), (pattern, dn)
        for rule, _ in ci.RULES + ci.EXCEPTIONS:                 # ... nor a rule of scripts/check_isa.py
            assert not re.search(rule, dn), (rule, dn)
