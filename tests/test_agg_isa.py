"""ISA of the aggregation kernels (csrc/kernels/agg.hip) in the shipped library, read the way scripts/check_isa.py reads the
row kernels (its helpers, its rules untouched): no scratch, and the neighbour rows of a batch issued back to back — at
least 4 row loads with no `s_waitcnt vmcnt` between them, 16-byte loads in the 16-byte instantiations."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_agg_kernels_keep_row_loads_in_flight_without_scratch(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from wholegraph_amd import binding
    seen = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(r"(agg_forward_kernel|agg_bwd_chunk_kernel|agg_bwd_fold_kernel)<(\d), (\d+)>", dn)
                if not m or "[clone" in dn:
                    continue
                vec = int(m.group(2))
                loads = ci.analyse(lines, wide=(vec == 4))[0]
                _, spilled, scratch = meta[mangled]
                seen[m.group(0)] = (loads, spilled, scratch)
    want = {"%s<%d, %d>" % (k, v, l) for k in ("agg_forward_kernel", "agg_bwd_chunk_kernel", "agg_bwd_fold_kernel")
            for v in (1, 4) for l in (16, 32, 64)}
    assert set(seen) == want, sorted(want - set(seen))
    bad = {k: v for k, v in seen.items() if v[0] < 4 or v[1] != 0 or v[2] != 0}
    assert not bad, "(loads in flight, spilled VGPRs, scratch bytes): %s" % bad
