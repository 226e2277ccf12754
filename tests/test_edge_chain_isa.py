"""ISA of the edge attribute gather kernel (csrc/kernels/graph.hip) in the shipped library, read with the helpers of
scripts/check_isa.py: every instantiation the launcher can reach is present, none has scratch or spilled VGPRs, none holds an
atomic, and its scalar memory instructions only read. The sampling kernels next to it are handed an edge id pointer at run
time and are not edited: the set of their instantiations is the one the dispatch reached before, still without scratch."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_isa():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    return ci


def _kernels(pattern):
    """{demangled name: (ISA lines, (vgprs, spilled vgprs, scratch bytes))} of the kernels whose name matches"""
    ci = _check_isa()
    from wholegraph_amd import binding
    out = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                if "[clone" in dn or mangled not in meta:
                    continue
                m = re.search(pattern, dn)
                if m:
                    out[m.group(0)] = (lines, meta[mangled])
    return out


def test_edge_attr_gather_kernel_has_no_scratch_no_spills_and_plain_memory_operations(wm_lib):
    ci = _check_isa()
    seen = _kernels(r"\bedge_attr_gather_kernel<\d+>")
    assert set(seen) == {"edge_attr_gather_kernel<%d>" % k for k in (1, 2, 4, 8)}, sorted(seen)
    bad = {k: v[1] for k, v in seen.items() if v[1][1] != 0 or v[1][2] != 0}
    assert not bad, "(VGPRs, spilled VGPRs, scratch bytes): %s" % bad
    # no name-pattern rule of the row-kernel gate claims the new kernel
    assert not [pat for pat, _ in ci.RULES if re.search(pat, "edge_attr_gather_kernel<4>")]
    for name, (lines, _) in seen.items():
        ops = [ln.split()[0] for ln in lines if ln.split()]
        assert any(op.startswith("global_load_dwordx2") for op in ops), name            # the 8-byte edge ids
        assert any(op.startswith("global_store_dword") for op in ops), name
        assert not [op for op in ops if "atomic" in op], name
        # scalar memory instructions only read (the kernel arguments, the per-rank tables of a chunked mapping)
        assert not [op for op in ops if op.startswith("s_") and ("store" in op or "dcache" in op)], name
        assert not [op for op in ops if op.startswith(("scratch_", "buffer_"))], name


def test_sampling_kernels_keep_their_instantiations_without_scratch(wm_lib):
    ids = ("int", "long")
    want = {"sample_small_kernel<%s, %s, %s>" % (i, c, g) for i in ids for c in ids for g in ("32", "64")}
    want |= {"sample_%s_kernel<%s, %s>" % (k, i, c) for k in ("sparse", "large") for i in ids for c in ids}
    want |= {"sample_weighted_kernel<%s, %s, %s>" % (i, c, w) for i in ids for c in ids for w in ("float", "double")}
    want |= {"sample_weighted_small_kernel<%s, %s, %s, %s>" % (i, c, w, g) for i in ids for c in ids for w in ("float", "double")
             for g in ("32", "64")}
    seen = _kernels(r"\bsample_(small|sparse|large|weighted|weighted_small)_kernel<[^>]*>")
    assert set(seen) == want, (sorted(want - set(seen)), sorted(set(seen) - want))
    # (sample_weighted_kernel keeps its candidate list in LDS and sample_large_kernel its slots in the output: neither spills)
    bad = {k: v[1] for k, v in seen.items() if v[1][1] != 0 or v[1][2] != 0}
    assert not bad, "(VGPRs, spilled VGPRs, scratch bytes): %s" % bad
