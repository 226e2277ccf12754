"""ISA of the table-reading aggregation kernels (csrc/kernels/agg_gather.hip) in the shipped library, read with
scripts/check_isa.py's helpers (its rules untouched) at the bar tests/test_agg_half_isa.py sets: no scratch, no spilled
VGPRs, and the rows of a batch issued back to back — at least 4 row loads with no `s_waitcnt vmcnt` between them,
`global_load_dwordx4` in the 16-byte instantiations, any `global_load_` in the element-wise ones. The row addresses come out
of shuffles as integers: a flat load there would count on the shuffles' counter too, so none is allowed. The set of
instantiations found is the set the dispatch can reach: {fp32 (4 floats a piece), fp16, bf16 (8 elements a piece)} x
{16-byte pieces, element-wise} x {16, 32, 64} lanes."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = r"\b(aggg_forward_kernel)<(?:wm::)?(float|f16_rows|bf16_rows), (\d+), (\d+)>"


def _check_isa():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    return ci


def test_aggg_kernels_keep_row_loads_in_flight_without_scratch(wm_lib):
    ci = _check_isa()
    from wholegraph_amd import binding
    seen = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(PATTERN, dn)
                if not m or "[clone" in dn:
                    continue
                assert mangled in meta, dn
                vec = int(m.group(3))
                loads = ci.analyse(lines, wide=(vec > 1))[0]
                flat = sum(1 for ln in lines if ln.split()[0].startswith("flat_load"))
                atomics = sum(1 for ln in lines if "atomic" in ln.split()[0])
                _, spilled, scratch = meta[mangled]
                seen["%s<%s, %d, %s>" % (m.group(1), m.group(2), vec, m.group(4))] = (loads, spilled, scratch, flat, atomics)
    want = {"aggg_forward_kernel<%s, %d, %d>" % (t, v, l)
            for t, vecs in (("float", (4, 1)), ("f16_rows", (8, 1)), ("bf16_rows", (8, 1))) for v in vecs for l in (16, 32, 64)}
    assert len(want) == 18
    assert set(seen) == want, (sorted(want - set(seen)), sorted(set(seen) - want))
    bad = {k: v for k, v in seen.items() if v[0] < 4 or v[1:] != (0, 0, 0, 0)}
    assert not bad, "(loads in flight, spilled VGPRs, scratch bytes, flat loads, atomics): %s" % bad


def test_aggg_names_stay_outside_the_other_kernel_patterns():
    """the fp32, 16-bit and weighted ISA tests count `agg_*`, `agg16_*` and `aggw_*` instantiations and check_isa.py's rule
    table matches kernels by name: the new template must fall under none of them"""
    ci = _check_isa()
    for t in ("float", "wm::f16_rows", "wm::bf16_rows"):
        for v in (1, 4, 8):
            name = "void wm::(anonymous namespace)::aggg_forward_kernel<%s, %d, 16>(wm::(anonymous namespace)::aggg_params)" % (t, v)
            assert not re.search(r"(agg_forward_kernel|agg_bwd_chunk_kernel|agg_bwd_fold_kernel)<(\d), (\d+)>", name)
            assert not re.search(r"\bagg_forward_kernel<4, 64>", name)
            assert not re.search(r"\b(agg16_\w+_kernel)<", name)
            assert not re.search(r"\b(aggw_\w+_kernel)<(\d), (\d+)>", name)
            assert not re.search(r"\b(gat_\w+_kernel)(<(\d)(, (\d+))?>)?\(", name)
            assert not any(re.search(pat, name) for pat, _ in ci.RULES)
