"""Weighted sampling on the fused hop and the one-call chain, without a GPU: the keyword arguments of the Python surface, the
two entry points in header / export list / bindings, and the argument checks that answer before any device work (plain host
tensors wrapped as wholememory tensors: nothing here may reach a kernel)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wholememory_ext_weighted_sample_append_unique", "wholememory_ext_multilayer_sample_weighted")
INVALID_INPUT = 6


def test_keyword_arguments(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import graph_structure, wholegraph_ops
    for fn in (wholegraph_ops.sample_append_unique, wholegraph_ops.multilayer_sample_begin, wholegraph_ops.multilayer_sample):
        p = inspect.signature(fn).parameters["wm_csr_weight_ptr_tensor"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    # positional use stays as it was
    assert list(inspect.signature(wholegraph_ops.sample_append_unique).parameters)[:5] == [
        "wm_csr_row_ptr_tensor", "wm_csr_col_ptr_tensor", "center_nodes_tensor", "max_sample_count", "random_seed"]
    assert list(inspect.signature(wholegraph_ops.multilayer_sample).parameters)[:5] == [
        "wm_csr_row_ptr_tensor", "wm_csr_col_ptr_tensor", "seed_nodes_tensor", "max_sample_counts", "random_seeds"]
    begin = inspect.signature(wgth.GraphStructure.multilayer_sample_begin).parameters
    assert begin["weight_name"].kind is inspect.Parameter.KEYWORD_ONLY and begin["weight_name"].default is None
    assert list(begin)[:3] == ["self", "node_ids", "max_neighbors"]
    sample = inspect.signature(wgth.GraphStructure.multilayer_sample_without_replacement).parameters
    assert list(sample)[:4] == ["self", "node_ids", "max_neighbors", "weight_name"]
    assert callable(graph_structure._DeferredSample.result)


def test_symbols_declared_exported_bound(wm_lib):
    from wholegraph_amd import binding
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared" % name
        assert name in exported, "%s is not exported" % name
        assert name in binding.PROTOTYPES, "%s is not bound" % name
    # one more tensor argument than the unweighted entry points
    for new, old in zip(NEW, ("wholememory_ext_sample_append_unique", "wholememory_ext_multilayer_sample")):
        assert len(binding.PROTOTYPES[new][1]) == len(binding.PROTOTYPES[old][1]) + 1


def _host_graph():
    import torch
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    t = dict(row=torch.tensor([0, 2, 4, 4], dtype=torch.int64), col=torch.tensor([1, 2, 0, 2], dtype=torch.int64),
             w=torch.tensor([1.0, 2.0, 0.5, 4.0]), wd=torch.tensor([1.0, 2.0, 0.5, 4.0], dtype=torch.float64),
             wint=torch.tensor([1, 2, 3, 4], dtype=torch.int32), wshort=torch.ones(3), centers=torch.tensor([0, 1, 2]),
             centers32=torch.tensor([0, 1, 2], dtype=torch.int32), offsets=torch.zeros(4, dtype=torch.int32))
    return {k: wrap_torch_tensor(v) for k, v in t.items()}


def test_fused_hop_validates_arguments(wm_lib):
    """every answer here comes before the first allocation or launch"""
    from wholegraph_amd import binding
    L, g = wm_lib, _host_graph()
    env = L.wholememory_get_default_env_func()
    ctx = C.c_void_p(1)   # a non-null memory context that is never used: every call below is turned down first
    ok = dict(row=g["row"].handle, col=g["col"].handle, w=g["w"].handle, centers=g["centers"].handle, m=2,
              offsets=g["offsets"].handle, uniq=ctx, pos=ctx, lid=ctx, env=env)

    def call(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_weighted_sample_append_unique(a["row"], a["col"], a["w"], a["centers"], a["m"], 7, a["offsets"],
                                                               a["uniq"], a["pos"], a["lid"], a["env"], None)

    for name in ("row", "col", "w", "centers", "offsets", "uniq", "pos", "lid", "env"):
        assert call(**{name: None}) == INVALID_INPUT, name
    # what the unweighted hop declines ...
    assert call(m=0) == binding.NOT_SUPPORTED
    assert call(centers=g["centers32"].handle) == binding.NOT_SUPPORTED      # int32 frontier, int64 columns
    # ... and the weighted hop on top of it
    assert call(w=g["wint"].handle) == binding.NOT_SUPPORTED
    assert call(w=g["wshort"].handle) == binding.NOT_SUPPORTED
    assert call(m=8193) == binding.NOT_SUPPORTED


def test_chain_validates_arguments_and_answers_queries(wm_lib):
    from wholegraph_amd import binding
    L, g = wm_lib, _host_graph()
    fan = lambda *m: (C.c_int * len(m))(*m)

    def query(w, hops, fans, seeds=g["centers"].handle, row=g["row"].handle, col=g["col"].handle):
        return L.wholememory_ext_multilayer_sample_weighted(row, col, w, seeds, hops, fans, None, None, None, None, None, None,
                                                            None, None)

    assert query(g["w"].handle, 2, fan(30, 30)) == binding.WHOLEMEMORY_SUCCESS
    assert query(g["wd"].handle, 3, fan(5, 64, 8192)) == binding.WHOLEMEMORY_SUCCESS
    assert query(g["w"].handle, 2, fan(30, 8193)) == binding.NOT_SUPPORTED
    assert query(g["wint"].handle, 2, fan(30, 30)) == binding.NOT_SUPPORTED
    assert query(g["wshort"].handle, 2, fan(30, 30)) == binding.NOT_SUPPORTED
    assert query(g["w"].handle, 2, fan(30, 0)) == binding.NOT_SUPPORTED
    assert query(g["w"].handle, 2, fan(30, 30), seeds=g["centers32"].handle) == binding.NOT_SUPPORTED
    assert query(None, 2, fan(30, 30)) == INVALID_INPUT
    assert query(g["w"].handle, 0, fan(30)) == INVALID_INPUT
    assert query(g["w"].handle, 2, None) == INVALID_INPUT
    assert query(g["w"].handle, 2, fan(30, 30), seeds=None) == INVALID_INPUT
    assert query(g["w"].handle, 2, fan(30, 30), row=None) == INVALID_INPUT
    # the unweighted chain answers the same query as before, fan-outs above 8192 included
    assert L.wholememory_ext_multilayer_sample(g["row"].handle, g["col"].handle, g["centers"].handle, 2, fan(30, 8193), None, None,
                                               None, None, None, None, None, None) == binding.WHOLEMEMORY_SUCCESS
    # not a query (sample_offsets given) with the rest missing: refused before anything is queued
    ptrs = (C.c_void_p * 2)(None, None)
    assert L.wholememory_ext_multilayer_sample_weighted(g["row"].handle, g["col"].handle, g["w"].handle, g["centers"].handle, 2,
                                                        fan(30, 30), None, ptrs, None, None, None, None, None,
                                                        None) == INVALID_INPUT


_CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
os.environ["WHOLEGRAPH_AMD_TESTING"] = "1"
import torch
from wholegraph_amd import binding as wmb
from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
L = wmb.lib()
tb = C.CDLL(os.path.join(sys.argv[1], "oracle", "libwm_test_backend.so"))
tb.wm_test_backend.restype = C.c_void_p
wmb.check(L.wm_testing_install_backend(C.c_void_p(tb.wm_test_backend())))
assert L.wholememory_ext_backend_name().startswith(b"oracle-test-backend")
row = wrap_torch_tensor(torch.tensor([0, 2, 4, 4], dtype=torch.int64))
col = wrap_torch_tensor(torch.tensor([1, 2, 0, 2], dtype=torch.int64))
w = wrap_torch_tensor(torch.tensor([1.0, 2.0, 0.5, 4.0]))
centers = wrap_torch_tensor(torch.tensor([0, 1, 2]))
offsets = wrap_torch_tensor(torch.zeros(4, dtype=torch.int32))
env, ctx = L.wholememory_get_default_env_func(), C.c_void_p(1)
hop = L.wholememory_ext_weighted_sample_append_unique(row.handle, col.handle, w.handle, centers.handle, 2, 7, offsets.handle, ctx,
                                                      ctx, ctx, env, None)
fan = (C.c_int * 2)(30, 30)
chain = L.wholememory_ext_multilayer_sample_weighted(row.handle, col.handle, w.handle, centers.handle, 2, fan, None, None, None,
                                                     None, None, None, None, None)
print("RESULT", hop, chain)
'''


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    """a backend without the graph kernels: NOT_SUPPORTED from both entry points, no crash"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    hop, chain = (int(v) for v in line.split()[1:])
    from wholegraph_amd import binding
    assert hop == binding.NOT_SUPPORTED and chain == binding.NOT_SUPPORTED
