"""ISA of the 16-bit-row aggregation kernels (csrc/kernels/agg_half.hip) in the shipped library, read with
scripts/check_isa.py's helpers (its rules untouched) at the bar tests/test_agg_isa.py sets for the fp32 kernels: no scratch,
no spilled VGPRs, and the neighbour rows of a batch issued back to back — at least 4 row loads with no `s_waitcnt vmcnt`
between them, `global_load_dwordx4` in the 16-byte instantiations, any `global_load_` in the element-wise ones. The set of
instantiations found is the set the dispatch can reach: {fp16, bf16} x {8 elements a piece, element-wise} x {16, 32, 64}
lanes, for each of the forward, chunk and fold kernels."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("agg16_forward_kernel", "agg16_bwd_chunk_kernel", "agg16_bwd_fold_kernel")


def test_agg16_kernels_keep_row_loads_in_flight_without_scratch(wm_lib):
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
                m = re.search(r"\b(agg16_\w+_kernel)<(?:wm::)?(f16_rows|bf16_rows), (\d+), (\d+)>", dn)
                if not m or "[clone" in dn:
                    continue
                assert mangled in meta, dn
                vec = int(m.group(3))
                loads = ci.analyse(lines, wide=(vec == 8))[0]
                _, spilled, scratch = meta[mangled]
                seen["%s<%s, %d, %s>" % (m.group(1), m.group(2), vec, m.group(4))] = (loads, spilled, scratch)
    want = {"%s<%s, %d, %d>" % (k, t, v, l) for k in KERNELS for t in ("f16_rows", "bf16_rows") for v in (1, 8)
            for l in (16, 32, 64)}
    assert len(want) == 36
    assert set(seen) == want, (sorted(want - set(seen)), sorted(set(seen) - want))
    bad = {k: v for k, v in seen.items() if v[0] < 4 or v[1] != 0 or v[2] != 0}
    assert not bad, "(loads in flight, spilled VGPRs, scratch bytes): %s" % bad


def test_agg16_names_stay_outside_the_fp32_and_row_kernel_patterns():
    """the fp32 ISA test counts `agg_*_kernel<V, L>` instantiations and check_isa.py's rule table matches kernels by name:
    the 16-bit templates must fall under neither"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    for k in KERNELS:
        name = "void wm::(anonymous namespace)::%s<wm::bf16_rows, 8, 16>(wm_agg16_args)" % k
        assert not re.search(r"(agg_forward_kernel|agg_bwd_chunk_kernel|agg_bwd_fold_kernel)<(\d), (\d+)>", name)
        assert not any(re.search(pat, name) for pat, _ in ci.RULES)
