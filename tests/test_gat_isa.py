"""ISA of the GAT kernels (csrc/kernels/gat.hip) in the shipped library, read with scripts/check_isa.py's helpers (its
rules untouched): no gat_* instantiation uses scratch or spills VGPRs, and the row-pass kernels issue the neighbour rows
of a batch back to back — at least 4 row loads with no `s_waitcnt vmcnt` between them, 16-byte loads in the 16-byte
instantiations."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_PASS = ("gat_fwd_kernel", "gat_bwd_chunk_kernel", "gat_bwd_fold_kernel")


def test_gat_kernels_without_scratch_and_row_loads_in_flight(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from wholegraph_amd import binding
    seen, rows = {}, {}
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(r"\b(gat_\w+_kernel)(<(\d)(, (\d+))?>)?\(", dn)
                if not m or "[clone" in dn or mangled not in meta:
                    continue
                key = m.group(1) + (m.group(2) or "")
                _, spilled, scratch = meta[mangled]
                seen[key] = (spilled, scratch)
                if m.group(1) in ROW_PASS:
                    rows[key] = ci.analyse(lines, wide=(m.group(3) == "4"))[0]
    want_rows = {"%s<%d, %d>" % (k, v, l) for k in ROW_PASS for v in (1, 4) for l in (16, 32, 64)}
    assert set(rows) == want_rows, sorted(want_rows - set(rows))
    others = {"gat_score_kernel<1>", "gat_score_kernel<4>", "gat_bwd_edge_kernel<1>", "gat_bwd_edge_kernel<4>",
              "gat_head_mean_kernel", "gat_bwd_prep_kernel", "gat_att_chunk_kernel", "gat_att_fold_kernel"}
    assert want_rows | others <= set(seen), sorted((want_rows | others) - set(seen))
    bad = {k: v for k, v in seen.items() if v != (0, 0)}
    assert not bad, "(spilled VGPRs, scratch bytes): %s" % bad
    few = {k: v for k, v in rows.items() if v < 4}
    assert not few, "row loads in flight: %s" % few
