"""ISA of the relation-typed aggregation kernels (csrc/kernels/agg_rel.hip) in the shipped library, read with
scripts/check_isa.py's helpers (its rules untouched) at the bar tests/test_agg_weighted_isa.py sets for the weighted kernels:
no scratch, no spilled VGPRs, and the rows of a batch issued back to back — at least 4 row loads with no `s_waitcnt vmcnt`
between them, `global_load_dwordx4` in the 16-byte instantiations, any `global_load_` in the element-wise ones. The set of
instantiations found is the set the dispatch can reach: {16-byte pieces, element-wise} x {16, 32, 64} lanes for each of the
forward, chunk and fold kernels. No multiply-add may be fused: (2h) rounds every product on its own, so a kernel holds at
most the fused steps of ONE IEEE division's expansion (the forward's fl(1 / n_r(d)); the backward divides nothing)."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("relagg_fwd_kernel", "relagg_chunk_bwd_kernel", "relagg_fold_bwd_kernel")


def _check_isa():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    return ci


def _float_fma(lines):
    return sum(1 for ln in lines if ln.split() and re.match(r"v_(pk_)?(fma|fmac|mad|mac)(_legacy)?_f\d+", ln.split()[0]))


def test_relagg_kernels_keep_row_loads_in_flight_without_scratch(wm_lib):
    ci = _check_isa()
    from wholegraph_amd import binding
    seen, fused, division = {}, {}, None
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                if "[clone" in dn:
                    continue
                if re.search(r"\bagg_forward_kernel<4, 64>", dn):
                    division = _float_fma(lines)
                m = re.search(r"\b(relagg_\w+_kernel)<(\d), (\d+)>", dn)
                if not m:
                    continue
                assert mangled in meta, dn
                vec = int(m.group(2))
                loads = ci.analyse(lines, wide=(vec == 4))[0]
                _, spilled, scratch = meta[mangled]
                seen[m.group(0)] = (loads, spilled, scratch)
                fused[m.group(0)] = _float_fma(lines)
    want = {"%s<%d, %d>" % (k, v, l) for k in KERNELS for v in (1, 4) for l in (16, 32, 64)}
    assert len(want) == 18
    assert set(seen) == want, (sorted(want - set(seen)), sorted(set(seen) - want))
    bad = {k: v for k, v in seen.items() if v[0] < 4 or v[1] != 0 or v[2] != 0}
    assert not bad, "(loads in flight, spilled VGPRs, scratch bytes): %s" % bad
    # the one IEEE division of the forward (1 / edges of the relation) expands into a fixed sequence with fused steps of its
    # own: the unweighted forward, which multiplies nothing before an add, has exactly those. The backward kernels multiply
    # by the stored edge_scale and divide nothing: no fused step at all. Any more would be a product fused with its add.
    assert division is not None and division > 0
    for k, v in fused.items():
        allowed = division if k.startswith("relagg_fwd_kernel") else 0
        assert v == allowed, "float multiply-adds in %s: %d, the division sequence accounts for %d" % (k, v, allowed)


def test_relagg_names_stay_outside_the_existing_kernel_patterns():
    """the other ISA tests count `agg_*_kernel<V, L>` / `agg16_*` / `aggw_*` / gat-family instantiations and check_isa.py's
    rule table matches kernels by name: the relation-typed templates must fall under none of them"""
    ci = _check_isa()
    for k in KERNELS:
        name = "void wm::(anonymous namespace)::%s<4, 16>(wm_relagg_args)" % k
        assert not re.search(r"(agg_forward_kernel|agg_bwd_chunk_kernel|agg_bwd_fold_kernel)<(\d), (\d+)>", name)
        assert not re.search(r"\b(agg16_\w+_kernel)<", name)
        assert not re.search(r"\b(aggw_\w+_kernel)<", name)
        assert not re.search(r"\b(gather_agg\w*|gat_\w+|gatv2_\w+|gat_edge_\w+)<", name)
        assert not any(re.search(pat, name) for pat, _ in ci.RULES)
