"""The induced-subgraph surface without a GPU: the C entry point (declared in section 2q of the extension header, exported,
bound), its argument checks on host tensors wrapped as wholememory tensors — every answer about the arguments before any device
work, in the order of sections 2m - 2o (shapes and sizes, then dtypes), pinned by calls with two faults, under the product
backend and under the CPU test backend, which has no such kernels and answers NOT_SUPPORTED to a well-formed call; and the
names, signatures and Python-side errors of wholegraph_ops.induced_subgraph, GraphStructure.induced_subgraph,
GraphStructure.saint_random_walk_subgraph and SubgraphGNNModel."""
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wholememory_ext_csr_induced_subgraph"
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_symbol_declared_exported_and_bound(wm_lib):
    import ctypes as C
    from wholegraph_amd import binding
    restype, argtypes = binding.PROTOTYPES[NAME]
    assert restype is C.c_int and len(argtypes) == 8
    assert all(argtypes[i] is C.c_void_p for i in (0, 1, 2, 3, 4, 5, 7))
    assert argtypes[6] is C.POINTER(binding.EnvFunc)
    assert hasattr(wm_lib, NAME)
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())


def test_header_states_the_op_between_2p_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2q)") == 1
    p2, q2, seam = text.index("---- (2p)"), text.index("---- (2q)"), text.index("---- (3) testing seam")
    assert p2 < q2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2q)") == 1 and head.index("(2p)") < head.index("(2q)") < head.index("(3) the testing seam")
    assert text.count(NAME + "(") == 1 and q2 < text.index(NAME + "(") < seam
    declaration = " ".join(re.sub(r"/\*.*?\*/", " ", text[text.index(NAME + "("):seam].split(";")[0]).split())   # (without comments)
    assert declaration.replace("( ", "(") == (
        NAME + "(wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, "
        "wholememory_tensor_t nodes_tensor, wholememory_tensor_t output_offset_tensor, void* output_col_memory_context, "
        "void* output_edge_gid_memory_context, wholememory_env_func_t* p_env_fns, void* stream)"), declaration
    section = " ".join(text[q2:seam].replace("\n *", "\n").split())
    for words in ("as (2m)", "A node v is a member when 0 <= v < n_nodes and v occurs in nodes",
                  "Its local id is first(v), the lowest i with nodes[i] == v",
                  "Duplicates in nodes are allowed: every position gets a row",
                  "the row is empty when u is outside [0, n_nodes)",
                  "does not satisfy 0 <= s <= e <= n_edges and e - s < 2^31",
                  "for pos = s .. e - 1 ascending with c = col_ind[pos]: if c is a member, the row gets the entry (first(c), pos)",
                  "Multi-edges and self-loops are kept", "the graph's order within a row is kept",
                  "offsets is the exclusive prefix of the row lengths, offsets[n] = m",
                  "col[k] is the local id of entry k, edge_gid[k] its position in col_ind",
                  "only ever compared, never used as an index", "damaged entries (-1, n_nodes, 2^31 - 1) never match",
                  "because such values are not members", "a function of the graph and nodes alone",
                  "one host round trip, for m", "wholememory_ext_set_async_completion",
                  "n >= 2^31 - 1", "fewer than n + 1 entries", "offsets not int32", "HIERARCHY", "NOT_IMPLEMENTED",
                  "every membership probe would be a collective gather", "NOT_SUPPORTED",
                  "m >= 2^31: answered after the count, with no output allocated",
                  "n = 0 succeeds: it writes offsets[0] = 0 and allocates empty outputs"):
        assert words in section, words


def test_python_names_and_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    import pylibwholegraph.torch as alias
    from wholegraph_amd.torch import saint, wholegraph_ops
    E = inspect.Parameter.empty
    KW, POS = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = inspect.signature(wholegraph_ops.induced_subgraph)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("wm_csr_row_ptr_tensor", E, POS), ("wm_csr_col_ptr_tensor", E, POS), ("nodes_tensor", E, POS),
        ("need_edge_output", False, KW)]
    sig = inspect.signature(wgth.GraphStructure.induced_subgraph)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("nodes", E, POS), ("need_edge_output", False, KW), ("edge_attr_names", None, KW)]
    sig = inspect.signature(wgth.GraphStructure.saint_random_walk_subgraph)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("roots", E, POS), ("walk_length", E, POS), ("random_seed", None, KW), ("weight_name", None, KW),
        ("need_edge_output", False, KW)]
    sig = inspect.signature(saint.SubgraphGNNModel.__init__)
    assert [p.name for p in sig.parameters.values()] == ["self", "graph_structure", "node_embedding", "args"]
    sig = inspect.signature(saint.SubgraphGNNModel.forward)
    assert [p.name for p in sig.parameters.values()] == ["self", "nodes", "offsets", "col"]
    # exported the way negative_sample is: the module and the class, and through the pylibwholegraph.torch alias
    assert wgth.wholegraph_ops.induced_subgraph is wholegraph_ops.induced_subgraph
    assert alias.wholegraph_ops.induced_subgraph is wholegraph_ops.induced_subgraph
    assert alias.GraphStructure.induced_subgraph is wgth.GraphStructure.induced_subgraph
    assert alias.GraphStructure.saint_random_walk_subgraph is wgth.GraphStructure.saint_random_walk_subgraph
    assert wgth.SubgraphGNNModel is saint.SubgraphGNNModel and alias.SubgraphGNNModel is saint.SubgraphGNNModel
    assert alias.saint is saint and "SubgraphGNNModel" in wgth.__all__ and "saint" in wgth.__all__
    # HomoGNNModel's refusal of "gat" stands; the subgraph model builds that model's layers itself
    wgth.set_framework("cugraph")
    with pytest.raises(NotImplementedError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gat")


def test_python_side_errors_come_before_the_library(wm_lib, monkeypatch):
    import types
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    from wholegraph_amd.torch import wholegraph_ops
    monkeypatch.setattr(binding, "lib", lambda: pytest.fail("reached the library"))
    nodes = torch.zeros(4, dtype=torch.int64)
    for bad in (nodes.reshape(2, 2), nodes[0], nodes.reshape(4, 1)):
        for edges in (False, True):
            with pytest.raises(ValueError, match="1-D"):
                wholegraph_ops.induced_subgraph(None, None, bad, need_edge_output=edges)
    g = wgth.GraphStructure()
    g.csr_row_ptr = g.csr_col_ind = types.SimpleNamespace(wmb_tensor=None)
    with pytest.raises(ValueError, match="1-D"):
        g.induced_subgraph(nodes.reshape(2, 2))
    with pytest.raises(ValueError, match="1-D"):
        g.induced_subgraph(nodes.reshape(2, 2), need_edge_output=True, edge_attr_names=["__edge_id__"])
    with pytest.raises(AssertionError, match="no edge attribute named"):
        g.induced_subgraph(nodes, edge_attr_names=["missing"])
    with pytest.raises(ValueError, match="walk_length"):      # (the walk's own check, also before the library)
        g.saint_random_walk_subgraph(nodes, 0, random_seed=1)
    with pytest.raises(ValueError, match="1-D"):
        g.saint_random_walk_subgraph(nodes.reshape(2, 2), 3)


_CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
os.environ["WHOLEGRAPH_AMD_TESTING"] = "1"
import numpy as np
from wholegraph_amd import binding as wmb
L = wmb.lib()
if sys.argv[2] == "oracle":
    tb = C.CDLL(os.path.join(sys.argv[1], "oracle", "libwm_test_backend.so"))
    tb.wm_test_backend.restype = C.c_void_p
    wmb.check(L.wm_testing_install_backend(C.c_void_p(tb.wm_test_backend())))
    assert L.wholememory_ext_backend_name().startswith(b"oracle-test-backend")
else:
    assert L.wholememory_ext_backend_name() == b"hip-gfx950"
DT = {np.dtype(np.int32): wmb.DT_INT, np.dtype(np.int64): wmb.DT_INT64, np.dtype(np.float32): wmb.DT_FLOAT,
      np.dtype(np.int16): wmb.DT_INT16}
keep = []
def wrap(a, shape=None):
    """a host array as a wholememory tensor (nothing here reaches the point where its memory would be read); shape: what the
    description claims, whatever the array holds"""
    a = np.ascontiguousarray(a)
    keep.append(a)
    desc = wmb.make_tensor_desc(list(a.shape if shape is None else shape), DT[a.dtype])
    h = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(h), C.c_void_p(a.ctypes.data), C.byref(desc)))
    return h
n_nodes, n_edges, n = 5, 7, 4
i64, i32, f32, i16 = np.int64, np.int32, np.float32, np.int16
env = wmb.EnvFunc()          # (never called: every answer here comes before the first allocation)
ctx = C.c_void_p(1)          # (a memory context is opaque to the library and only handed to the env functions)
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), nodes=wrap(np.zeros(n, i64)),
          off=wrap(np.zeros(n + 1, i32)), cctx=ctx, ectx=None, env=C.byref(env))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_induced_subgraph(a["row"], a["col"], a["nodes"], a["off"], a["cctx"], a["ectx"], a["env"], None)
huge = (1 << 31) - 1      # (a description of 2^31 - 1 nodes over a one-entry array: refused before anything is read)
row32, colf, nodesf, off64 = wrap(np.zeros(n_nodes + 1, i32)), wrap(np.zeros(n_edges, f32)), wrap(np.zeros(n, f32)), wrap(np.zeros(n + 1, i64))
invalid = [call(row=None), call(col=None), call(nodes=None), call(off=None), call(cctx=None), call(env=None),
           call(row=wrap(np.zeros((2, 3), i64))), call(col=wrap(np.zeros((7, 1), i64))), call(nodes=wrap(np.zeros((2, 2), i64))),
           call(off=wrap(np.zeros((n + 1, 1), i32))),
           call(nodes=wrap(np.zeros(1, i64), [huge]), off=wrap(np.zeros(1, i32), [huge + 1])),       # n = 2^31 - 1
           call(nodes=wrap(np.zeros(1, i64), [1 << 40]), off=wrap(np.zeros(1, i32), [(1 << 40) + 1])),
           call(off=wrap(np.zeros(n, i32))), call(off=wrap(np.zeros(0, i32))),                         # shorter than n + 1
           # two faults, one of shape or size and one of dtype: the shape's answer
           call(nodes=wrap(np.zeros((2, 2), i64)), row=row32), call(cctx=None, col=colf), call(env=None, nodes=nodesf),
           call(off=wrap(np.zeros(n, i64))), call(off=wrap(np.zeros(n, i32)), row=row32),
           call(nodes=wrap(np.zeros(1, f32), [huge]), off=wrap(np.zeros(1, i32), [huge + 1])),
           call(col=wrap(np.zeros((7, 1), f32))), call(row=None, off=off64)]
logic = [call(row=row32), call(row=wrap(np.zeros(n_nodes + 1, f32))), call(col=colf), call(col=wrap(np.zeros(n_edges, i16))),
         call(nodes=nodesf), call(nodes=wrap(np.zeros(n, i16))), call(off=off64), call(off=wrap(np.zeros(n + 1, f32))),
         # two dtype faults; and a dtype fault with the edge-id context given
         call(row=row32, off=off64), call(col=colf, nodes=nodesf), call(off=off64, ectx=ctx)]
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [call(), call(ectx=ctx), call(nodes=wrap(np.zeros(n, i32))), call(col=wrap(np.zeros(n_edges, i32))),
            call(nodes=wrap(np.zeros(n, i32)), col=wrap(np.zeros(n_edges, i32))), call(off=wrap(np.zeros(n + 9, i32))),
            call(col=wrap(np.zeros(0, i64))), call(nodes=wrap(np.zeros(0, i64)), off=wrap(np.zeros(1, i32))),
            call(nodes=wrap(np.zeros(1, i64), [huge - 1]), off=wrap(np.zeros(1, i32), [huge]))]       # n = 2^31 - 2 is a size it takes
print("RESULT", len(invalid), len(logic), *invalid, *logic, *good)
'''


def _child(backend):
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, backend], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    a, b, *codes = (int(v) for v in line.split()[1:])
    return codes[:a], codes[a:a + b], codes[a + b:]


def test_argument_checks_and_not_supported_under_the_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    from wholegraph_amd import binding
    invalid, logic, good = _child("oracle")
    assert len(invalid) == 22 and invalid == [INV] * 22        # (the argument checks come first, whatever the backend)
    assert len(logic) == 11 and logic == [LOGIC] * 11
    assert good == [binding.NOT_SUPPORTED] * 9                  # no such kernels in that backend: nothing queued


def test_argument_checks_under_the_product_backend(wm_lib):
    """the same malformed calls with the product's backend installed and no device: answered before any device work"""
    invalid, logic, good = _child("hip")
    assert invalid == [INV] * 22 and logic == [LOGIC] * 11 and good == []
