"""Edge ids and edge attributes on the fused hop and the one-call chain, without a GPU: the keyword arguments of the Python
surface and their defaults, the three entry points in header / export list / bindings, the argument checks that answer before
any device work (plain host tensors wrapped as wholememory tensors: nothing here may reach a kernel), and NOT_SUPPORTED from
a backend without the graph kernels."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wholememory_ext_sample_append_unique_edges", "wholememory_ext_multilayer_sample_edges", "wholememory_ext_edge_chain_calls")
INVALID_INPUT = 6


def test_keyword_arguments_and_defaults(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import wholegraph_ops
    p = inspect.signature(wholegraph_ops.sample_append_unique).parameters["need_edge_output"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for fn in (wholegraph_ops.multilayer_sample_begin, wholegraph_ops.multilayer_sample):
        params = inspect.signature(fn).parameters
        assert params["need_edge_ids"].kind is inspect.Parameter.KEYWORD_ONLY and params["need_edge_ids"].default is False
        assert params["wm_edge_attr_tensors"].kind is inspect.Parameter.KEYWORD_ONLY and params["wm_edge_attr_tensors"].default is None
        assert params["wm_csr_weight_ptr_tensor"].kind is inspect.Parameter.KEYWORD_ONLY
    # positional use stays as it was
    assert list(inspect.signature(wholegraph_ops.sample_append_unique).parameters)[:5] == [
        "wm_csr_row_ptr_tensor", "wm_csr_col_ptr_tensor", "center_nodes_tensor", "max_sample_count", "random_seed"]
    assert list(inspect.signature(wholegraph_ops.multilayer_sample).parameters)[:5] == [
        "wm_csr_row_ptr_tensor", "wm_csr_col_ptr_tensor", "seed_nodes_tensor", "max_sample_counts", "random_seeds"]
    begin = inspect.signature(wgth.GraphStructure.multilayer_sample_begin).parameters
    assert begin["edge_attr_names"].kind is inspect.Parameter.KEYWORD_ONLY and begin["edge_attr_names"].default is None
    assert list(begin)[:3] == ["self", "node_ids", "max_neighbors"]
    with_attrs = inspect.signature(wgth.GraphStructure.multilayer_sample_with_edge_attributes).parameters
    assert list(with_attrs) == ["self", "node_ids", "max_neighbors", "edge_attr_names", "weight_name", "random_seeds"]
    assert with_attrs["random_seeds"].kind is inspect.Parameter.KEYWORD_ONLY and with_attrs["weight_name"].default is None


def test_return_arity_without_the_keywords_is_unchanged(wm_lib):
    """a finished chain hands out five entries per hop unless edge ids / attributes were asked for"""
    import torch
    from wholegraph_amd.torch import wholegraph_ops as wops

    class NoWait:
        def synchronize(self):
            pass

    def pending(edge_ids, edge_attrs):
        counts = torch.tensor([3, 2, 4, 1], dtype=torch.int32)
        offsets = [torch.zeros(3, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)]
        uniques = [torch.arange(8), torch.arange(40)]
        edges = [torch.zeros((2, 6), dtype=torch.int32), torch.zeros((2, 32), dtype=torch.int32)]
        p = wops.PendingMultilayerSample.__new__(wops.PendingMultilayerSample)
        p._hops, p._n0, p._offsets, p._uniques, p._edges, p._counts, p._result = 2, 2, offsets, uniques, edges, counts, None
        p._edge_ids, p._edge_attrs, p._stream, p._done, p.padded_frontier = edge_ids, edge_attrs, NoWait(), None, uniques[-1]
        return p

    plain = pending(None, None).finish()
    assert [len(hop) for hop in plain] == [5, 5]
    eids = [torch.arange(6), torch.arange(32)]
    with_ids = pending(eids, None).finish()
    assert [len(hop) for hop in with_ids] == [6, 6]
    assert with_ids[0][5].tolist() == [0, 1, 2] and with_ids[1][5].tolist() == [0, 1, 2, 3]
    attrs = [[torch.arange(6.0), torch.arange(6, dtype=torch.int32)], [torch.arange(32.0), torch.arange(32, dtype=torch.int32)]]
    with_attrs = pending(eids, attrs).finish()
    assert [len(hop) for hop in with_attrs] == [7, 7]
    assert [t.dtype for t in with_attrs[1][6]] == [torch.float32, torch.int32] and with_attrs[1][6][0].tolist() == [0.0, 1.0, 2.0, 3.0]
    for a, b in zip(plain, with_attrs):
        assert all(torch.equal(x, y) for x, y in zip(a, b[:5]))


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
    # the fused hop: the weighted one plus the edge id context; the chain: the weighted one plus edge_gid, n_attrs, attr_tensors, attr_out
    assert len(binding.PROTOTYPES[NEW[0]][1]) == len(binding.PROTOTYPES["wholememory_ext_weighted_sample_append_unique"][1]) + 1
    assert len(binding.PROTOTYPES[NEW[1]][1]) == len(binding.PROTOTYPES["wholememory_ext_multilayer_sample_weighted"][1]) + 4
    assert binding.PROTOTYPES[NEW[2]] == (C.c_int64, [])
    assert isinstance(wm_lib.wholememory_ext_edge_chain_calls(), int)


def _host_graph():
    import torch
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    t = dict(row=torch.tensor([0, 2, 4, 4], dtype=torch.int64), col=torch.tensor([1, 2, 0, 2], dtype=torch.int64),
             w=torch.tensor([1.0, 2.0, 0.5, 4.0]), wint=torch.tensor([1, 2, 3, 4], dtype=torch.int32),
             a64=torch.tensor([5, 6, 7, 8], dtype=torch.int64), ad=torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64),
             a16=torch.ones(4, dtype=torch.float16), ashort=torch.ones(3), a2d=torch.ones((4, 2)),
             centers=torch.tensor([0, 1, 2]), centers32=torch.tensor([0, 1, 2], dtype=torch.int32),
             offsets=torch.zeros(4, dtype=torch.int32))
    return {k: wrap_torch_tensor(v) for k, v in t.items()}


def test_fused_hop_validates_arguments(wm_lib):
    """every answer here comes before the first allocation or launch"""
    from wholegraph_amd import binding
    L, g = wm_lib, _host_graph()
    env = L.wholememory_get_default_env_func()
    ctx = C.c_void_p(1)   # a non-null memory context that is never used: every call below is turned down first
    ok = dict(row=g["row"].handle, col=g["col"].handle, w=g["w"].handle, centers=g["centers"].handle, m=2,
              offsets=g["offsets"].handle, uniq=ctx, pos=ctx, lid=ctx, egid=ctx, env=env)

    def call(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_sample_append_unique_edges(a["row"], a["col"], a["w"], a["centers"], a["m"], 7, a["offsets"],
                                                            a["uniq"], a["pos"], a["lid"], a["egid"], a["env"], None)

    for name in ("row", "col", "centers", "offsets", "uniq", "pos", "lid", "egid", "env"):
        assert call(**{name: None}) == INVALID_INPUT, name
        assert call(w=None, **{name: None}) == INVALID_INPUT, name
    # what the fused hops decline, weighted (a weight tensor) and unweighted (NULL)
    for w in (g["w"].handle, None):
        assert call(w=w, m=0) == binding.NOT_SUPPORTED
        assert call(w=w, centers=g["centers32"].handle) == binding.NOT_SUPPORTED      # int32 frontier, int64 columns
    assert call(w=g["wint"].handle) == binding.NOT_SUPPORTED
    assert call(w=g["ashort"].handle) == binding.NOT_SUPPORTED
    assert call(m=8193) == binding.NOT_SUPPORTED


def test_chain_validates_arguments_and_answers_queries(wm_lib):
    from wholegraph_amd import binding
    L, g = wm_lib, _host_graph()
    fan = lambda *m: (C.c_int * len(m))(*m)
    tensors = lambda *names: (C.c_void_p * len(names))(*[g[n].handle.value if n else None for n in names])
    base = dict(row=g["row"].handle, col=g["col"].handle, w=None, seeds=g["centers"].handle, hops=2, fans=fan(30, 30), rng=None,
                offsets=None, unique=None, pos=None, lid=None, egid=None, n_attrs=0, attrs=None, attr_out=None, counts=None,
                env=None)

    def call(**over):
        a = dict(base, **over)
        return L.wholememory_ext_multilayer_sample_edges(a["row"], a["col"], a["w"], a["seeds"], a["hops"], a["fans"], a["rng"],
                                                         a["offsets"], a["unique"], a["pos"], a["lid"], a["egid"], a["n_attrs"],
                                                         a["attrs"], a["attr_out"], a["counts"], a["env"], None)

    # queries: unweighted (NULL weights) and weighted, with and without attributes of every supported element type
    assert call() == binding.WHOLEMEMORY_SUCCESS
    assert call(w=g["w"].handle, hops=3, fans=fan(5, 10, 15)) == binding.WHOLEMEMORY_SUCCESS
    assert call(n_attrs=4, attrs=tensors("w", "wint", "a64", "ad")) == binding.WHOLEMEMORY_SUCCESS
    assert call(w=g["w"].handle, n_attrs=1, attrs=tensors("w")) == binding.WHOLEMEMORY_SUCCESS
    assert call(n_attrs=9, attrs=tensors(*["w", "a64", "ad"] * 3)) == binding.WHOLEMEMORY_SUCCESS    # more than one launch per hop
    # a query declines attribute tensors the kernel does not take: 2-byte elements, not one entry per edge, 2-D
    for bad in ("a16", "ashort", "a2d"):
        assert call(n_attrs=2, attrs=tensors("w", bad)) == binding.NOT_SUPPORTED, bad
    # ... and what the chains without edge ids decline
    assert call(fans=fan(30, 0)) == binding.NOT_SUPPORTED
    assert call(seeds=g["centers32"].handle) == binding.NOT_SUPPORTED
    assert call(w=g["w"].handle, fans=fan(30, 8193)) == binding.NOT_SUPPORTED
    assert call(fans=fan(30, 8193)) == binding.WHOLEMEMORY_SUCCESS                 # unweighted: no fan-out limit
    assert call(w=g["wint"].handle) == binding.NOT_SUPPORTED
    # INVALID_INPUT before any device work
    assert call(n_attrs=-1) == INVALID_INPUT
    assert call(n_attrs=1, attrs=None) == INVALID_INPUT
    assert call(n_attrs=2, attrs=tensors("w", None)) == INVALID_INPUT
    assert call(hops=0, fans=fan(30)) == INVALID_INPUT
    assert call(fans=None) == INVALID_INPUT
    assert call(seeds=None) == INVALID_INPUT
    assert call(row=None) == INVALID_INPUT
    ptrs = (C.c_void_p * 2)(None, None)
    counts = (C.c_int * 4)()
    env = L.wholememory_get_default_env_func()
    rng = (C.c_ulonglong * 2)(1, 2)
    full = dict(rng=rng, offsets=ptrs, unique=ptrs, pos=ptrs, lid=ptrs, counts=counts, env=env)
    # not a query: edge_gid == NULL, and attributes without attr_out
    assert call(**full) == INVALID_INPUT
    assert call(egid=ptrs, n_attrs=1, attrs=tensors("w"), **full) == INVALID_INPUT
    # not a query with the rest missing: refused as by the chain without edge ids
    assert call(offsets=ptrs, egid=ptrs) == INVALID_INPUT
    # none of this counted as a chain call
    assert L.wholememory_ext_edge_chain_calls() == 0


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
out = []
for weight in (None, w.handle):
    out.append(L.wholememory_ext_sample_append_unique_edges(row.handle, col.handle, weight, centers.handle, 2, 7, offsets.handle,
                                                            ctx, ctx, ctx, ctx, env, None))
    fan = (C.c_int * 2)(30, 30)
    out.append(L.wholememory_ext_multilayer_sample_edges(row.handle, col.handle, weight, centers.handle, 2, fan, None, None, None,
                                                         None, None, None, 0, None, None, None, None, None))
    attrs = (C.c_void_p * 1)(w.handle.value)
    out.append(L.wholememory_ext_multilayer_sample_edges(row.handle, col.handle, weight, centers.handle, 2, fan, None, None, None,
                                                         None, None, None, 1, attrs, None, None, None, None))
out.append(L.wholememory_ext_edge_chain_calls())
print("RESULT", *out)
'''


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    """a backend without the graph kernels: NOT_SUPPORTED from the fused hop and the chain with edge ids, no crash"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    got = [int(v) for v in line.split()[1:]]
    from wholegraph_amd import binding
    assert got[:-1] == [binding.NOT_SUPPORTED] * 6 and got[-1] == 0
