"""ISA of the edge-feature GAT kernels (csrc/kernels/gat_edge.hip) in the shipped library, read with scripts/check_isa.py's
helpers (its rules untouched), to the bar tests/test_gat_isa.py holds gat.hip's: no gat_edge_* instantiation uses scratch or
spills VGPRs. The 16-byte instantiations load and store 16 bytes at a time, the forward issues at least 4 neighbour rows of a
batch with no `s_waitcnt vmcnt` between them, and the edge-score kernel goes through LDS: edge_feat is read in memory order
(dwordx4 in the 16-byte instantiation) and walked per (edge, head) segment from there."""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def count(lines, pattern):
    pat = re.compile(pattern)
    return sum(1 for ln in lines if pat.match(ln))


def test_gat_edge_kernels(wm_lib):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import check_isa as ci
    finally:
        sys.path.pop(0)
    from wholegraph_amd import binding
    seen, code = {}, {}
    with tempfile.TemporaryDirectory() as wd:
        for co in ci.extract_code_object(binding.LIB_PATH, wd):
            funcs = ci.split_functions(ci.disassemble(co))
            meta = ci.kernel_metadata(co)
            names = ci.demangle(list(funcs))
            for mangled, lines in funcs.items():
                dn = names.get(mangled, mangled)
                m = re.search(r"\b(gat_edge_\w+_kernel)(<(\d)(, (\d+))?>)?\(", dn)
                if not m or "[clone" in dn or mangled not in meta:
                    continue
                key = m.group(1) + (m.group(2) or "")
                seen[key] = meta[mangled][1:]
                code[key] = lines
    fwd = {"gat_edge_fwd_kernel<%d, %d>" % (v, l) for v in (1, 4) for l in (16, 32, 64)}
    want = fwd | {"gat_edge_score_kernel<1>", "gat_edge_score_kernel<4>", "gat_edge_bwd_dz_kernel<1>",
                  "gat_edge_bwd_dz_kernel<4>", "gat_edge_grad_chunk_kernel<1>", "gat_edge_grad_chunk_kernel<4>",
                  "gat_edge_att_fold_kernel"}
    assert want <= set(seen), sorted(want - set(seen))
    bad = {k: v for k, v in seen.items() if v != (0, 0)}
    assert not bad, "(spilled VGPRs, scratch bytes): %s" % bad
    # the forward: the neighbour rows of a batch in flight together, as gat_fwd_kernel
    few = {k: ci.analyse(code[k], wide=k.startswith("gat_edge_fwd_kernel<4"))[0] for k in fwd}
    assert not {k: v for k, v in few.items() if v < 4}, "row loads in flight: %s" % few
    # 16-byte instantiations: 16-byte global loads (and stores where rows are written)
    for k in sorted(want):
        if "<4" not in k:
            continue
        assert count(code[k], r"^global_load_dwordx4\b") > 0, k
        if not k.startswith(("gat_edge_score_kernel", "gat_edge_bwd_dz_kernel")):   # (these write one float per segment)
            assert count(code[k], r"^global_store_dwordx4\b") > 0, k
    # the edge-score kernel stages edge_feat through LDS: written and read there, a barrier in between; its 16-byte
    # instantiation loads edge_feat with dwordx4 (checked above)
    for k in ("gat_edge_score_kernel<1>", "gat_edge_score_kernel<4>"):
        assert count(code[k], r"^ds_write") > 0 and count(code[k], r"^ds_read") > 0 and count(code[k], r"^s_barrier") > 0, k
