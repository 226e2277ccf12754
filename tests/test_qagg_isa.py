"""ISA of the aggregation kernels that read an 8-bit row-quantized table (csrc/kernels/agg_quant.hip) in the shipped library,
read with scripts/check_isa.py's helpers (its rules untouched) at the bar tests/test_gather_agg_isa.py sets: no scratch, no
spilled VGPRs, no atomics, and the rows of a batch issued back to back — at least 4 row loads (`global_load_dword`: a lane's
piece of a quantized row is one dword of codes) with no `s_waitcnt vmcnt` between them. The row addresses come out of
shuffles as integers: a flat load there would count on the shuffles' counter too, so none is allowed. The set of
instantiations found is the set the dispatch can reach: {one 16-byte store per lane, element-wise} x {16, 32, 64} lanes."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = r"\b(aggq_forward_kernel)<(\d+), (\d+)>"


def _check_isa():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    return ci


def test_aggq_kernels_keep_row_loads_in_flight_without_scratch(wm_lib):
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
                loads = ci.analyse(lines, wide=False, load_re=r"^global_load_dword\b")[0]
                flat = sum(1 for ln in lines if ln.split()[0].startswith("flat_load"))
                atomics = sum(1 for ln in lines if "atomic" in ln.split()[0])
                lds = sum(1 for ln in lines if re.match(r"ds_(read|write|load|store)", ln.split()[0]))
                _, spilled, scratch = meta[mangled]
                seen["%s<%s, %s>" % m.groups()] = (loads, spilled, scratch, flat, atomics, lds)
    want = {"aggq_forward_kernel<%d, %d>" % (v, l) for v in (4, 1) for l in (16, 32, 64)}
    assert len(want) == 6
    assert set(seen) == want, (sorted(want - set(seen)), sorted(set(seen) - want))
    bad = {k: v for k, v in seen.items() if v[0] < 4 or v[1:] != (0, 0, 0, 0, 0)}
    assert not bad, "(loads in flight, spilled VGPRs, scratch bytes, flat loads, atomics, LDS accesses): %s" % bad


def test_aggq_names_stay_outside_the_other_kernel_patterns():
    """the fp32, 16-bit, weighted, table-reading, GAT and quantized-row ISA tests count their kernels by name and
    check_isa.py's rule table matches kernels by name: the new template must fall under none of them"""
    ci = _check_isa()
    for v in (1, 4):
        for lanes in (16, 32, 64):
            name = "void wm::(anonymous namespace)::aggq_forward_kernel<%d, %d>(wm::(anonymous namespace)::aggq_params)" % (v, lanes)
            assert re.search(PATTERN, name)
            assert not re.search(r"(agg_forward_kernel|agg_bwd_chunk_kernel|agg_bwd_fold_kernel)<(\d), (\d+)>", name)
            assert not re.search(r"\bagg_forward_kernel<", name)
            assert not re.search(r"\b(agg16_\w+_kernel)<", name)
            assert not re.search(r"\b(aggw_\w+_kernel)<(\d), (\d+)>", name)
            assert not re.search(r"\b(aggg_forward_kernel)<(?:wm::)?(float|f16_rows|bf16_rows), (\d+), (\d+)>", name)
            assert not re.search(r"\b(gat_\w+_kernel)(<(\d)(, (\d+))?>)?\(", name)
            assert not re.search(r"qrows_\w+", name)
            assert not any(re.search(pat, name) for pat, _ in ci.RULES)
