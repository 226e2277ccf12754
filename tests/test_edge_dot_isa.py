"""ISA of the edge dot-product kernels (csrc/kernels/edot.hip) in the shipped library, read with scripts/check_isa.py's
helpers (its rules untouched), to the bar tests/test_tconv_isa.py holds tconv.hip's: no edot_* instantiation uses scratch or
spills VGPRs, and the row-pass kernels of the 16-byte instantiations issue the rows of a batch back to back: at least 4 row
loads with no `s_waitcnt vmcnt` between them. The set of instantiations is exactly the expected one, and the kernel names
stay clear of the patterns the other ISA tests count."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_PASS = ("edot_fwd_kernel", "edot_bwd_dst_kernel", "edot_bwd_chunk_kernel", "edot_bwd_fold_kernel")
COUNTED = (r"\bagg\w*_kernel", r"\bgat_\w+", r"\bgatv2_\w+", r"\bgat_edge_\w+", r"\brelagg_", r"\baggw_", r"\bagg16_", r"\baggg_",
           r"\bqrows_", r"\btconv_\w+", r"\bpna_\w+")


def test_edot_kernels_without_scratch_and_row_loads_in_flight(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from wholegraph_amd import binding
    seen, rows, full = {}, {}, []
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(r"\b(edot_\w+_kernel)(<(\d)(, (\d+))?>)?\(", dn)
                if not m or "[clone" in dn or mangled not in meta:
                    continue
                key = m.group(1) + (m.group(2) or "")
                full.append(dn)
                _, spilled, scratch = meta[mangled]
                seen[key] = (spilled, scratch)
                if m.group(1) in ROW_PASS and m.group(3) == "4":
                    rows[key] = ci.analyse(lines, wide=True)[0]
    want_rows = {"%s<4, %d>" % (k, l) for k in ROW_PASS for l in (16, 32, 64)}
    assert set(rows) == want_rows, sorted(want_rows ^ set(rows))
    want = want_rows | {"%s<1, %d>" % (k, l) for k in ROW_PASS for l in (16, 32, 64)}
    assert set(seen) == want, sorted(want ^ set(seen))
    bad = {k: v for k, v in seen.items() if v != (0, 0)}
    assert not bad, "(spilled VGPRs, scratch bytes): %s" % bad
    few = {k: v for k, v in rows.items() if v < 4}
    assert not few, "row loads in flight: %s" % few
    # the existing ISA tests count what these patterns find: none of the new kernels may be among it
    for dn in full:
        for pattern in COUNTED:
            assert not re.search(pattern, dn), (pattern, dn)
