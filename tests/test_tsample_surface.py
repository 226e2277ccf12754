"""The temporal-sampler surface without a GPU: the C entry point (declared in section 2r of the extension header, exported,
bound), its argument checks on host tensors wrapped as wholememory tensors — every answer about the arguments before any device
work, in the order of sections 2m - 2o and 2q (shapes and sizes, then dtypes), pinned by calls with two faults, under the
product backend and under the CPU test backend, which has no such kernels and answers NOT_SUPPORTED to a well-formed call; and
the names, signatures and Python-side errors of wholegraph_ops.temporal_sample_without_replacement,
GraphStructure.temporal_sample_one_hop, GraphStructure.multilayer_temporal_sample, TimeEncoder and TemporalGNNModel."""
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wholememory_ext_csr_temporal_sample"
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_symbol_declared_exported_and_bound(wm_lib):
    import ctypes as C
    from wholegraph_amd import binding
    restype, argtypes = binding.PROTOTYPES[NAME]
    assert restype is C.c_int and len(argtypes) == 16
    assert all(argtypes[i] is C.c_void_p for i in (0, 1, 2, 3, 4, 10, 11, 12, 13, 15))
    assert [argtypes[i] for i in (5, 6, 7)] == [C.c_int] * 3 and argtypes[8] is C.c_longlong and argtypes[9] is C.c_ulonglong
    assert argtypes[14] is C.POINTER(binding.EnvFunc)
    assert hasattr(wm_lib, NAME)
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())


def test_header_states_the_op_between_2q_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2r)") == 1
    q2, r2, seam = text.index("---- (2q)"), text.index("---- (2r)"), text.index("---- (3) testing seam")
    assert q2 < r2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2r)") == 1 and head.index("(2q)") < head.index("(2r)") < head.index("(3) the testing seam")
    assert text.count(NAME + "(") == 1 and r2 < text.index(NAME + "(") < seam
    declaration = " ".join(re.sub(r"/\*.*?\*/", " ", text[text.index(NAME + "("):seam].split(";")[0]).split())   # (without comments)
    assert declaration.replace("( ", "(") == (
        NAME + "(wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, "
        "wholememory_tensor_t wm_csr_edge_time_tensor, wholememory_tensor_t center_nodes_tensor, "
        "wholememory_tensor_t center_times_tensor, int max_sample_count, int strategy, int inclusive, long long time_window, "
        "unsigned long long random_seed, wholememory_tensor_t output_offset_tensor, void* output_dest_memory_context, "
        "void* output_center_localid_memory_context, void* output_edge_gid_memory_context, wholememory_env_func_t* p_env_fns, "
        "void* stream)"), declaration
    section = " ".join(text[r2:seam].replace("\n *", "\n").split())
    for words in ("as (2m)", "edge_time int64 [n_edges], one entry per edge position", "center_times int64 [n]",
                  "the row is empty when u is outside [0, n_nodes)", "does not satisfy 0 <= s <= e <= n_edges and e - s < 2^31",
                  "a col_ind entry is copied, never used as an index", "ts = edge_time[s + j]",
                  "ts <= t when inclusive != 0, ts < t when inclusive == 0",
                  "time_window < 0, or (uint64)t - (uint64)ts <= (uint64)time_window", "there is no overflow case",
                  "c_i = E_i when max_sample_count <= 0", "else c_i = min(E_i, M)", "M > 64 is INVALID_INPUT",
                  "offsets is the exclusive prefix of the c_i, offsets[n] the total",
                  "the first 32-bit output of stream(seed, i, j + 1) of (2m)",
                  "the largest composite (uint64(r) << 32) | (0xFFFFFFFF - j)", "ties to the lowest j",
                  "An ineligible neighbour draws nothing and shifts no one else's draw",
                  "strategy 1 (last): the M eligible neighbours with the largest ts, ties to the lowest j",
                  "in ascending j, whatever the strategy and whether or not a selection took place",
                  "center_localid[k] = i, edge_gid[k] = s + j", "not on n or on the launch geometry",
                  "the first 100 centres of a batch of 512 equal a batch of those 100",
                  "one host round trip, for the total", "wholememory_ext_set_async_completion",
                  "max_sample_count > 64", "strategy not 0 or 1", "n >= 2^31 - 1", "edge_time not one entry per edge",
                  "center_times not n entries", "fewer than n + 1 entries", "edge_time or center_times not int64",
                  "offsets not int32", "HIERARCHY", "NOT_IMPLEMENTED", "Python composes that route", "NOT_SUPPORTED",
                  "reachable with max_sample_count <= 0 only: answered after the count, with no output allocated",
                  "n = 0 succeeds: it writes offsets[0] = 0 and allocates empty outputs"):
        assert words in section, words


def test_python_names_and_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    import pylibwholegraph.torch as alias
    from wholegraph_amd.torch import temporal, wholegraph_ops
    E = inspect.Parameter.empty
    KW, POS = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = inspect.signature(wholegraph_ops.temporal_sample_without_replacement)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("wm_csr_row_ptr_tensor", E, POS), ("wm_csr_col_ptr_tensor", E, POS), ("wm_csr_edge_time_tensor", E, POS),
        ("center_nodes_tensor", E, POS), ("center_times_tensor", E, POS), ("max_sample_count", E, POS), ("random_seed", None, POS),
        ("need_center_local_output", False, POS), ("need_edge_output", False, POS), ("strategy", "uniform", KW),
        ("inclusive", True, KW), ("time_window", None, KW)]
    sig = inspect.signature(wgth.GraphStructure.temporal_sample_one_hop)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("time_name", E, POS), ("center_nodes_tensor", E, POS), ("center_times_tensor", E, POS), ("max_sample_count", E, POS),
        ("strategy", "uniform", KW), ("inclusive", True, KW), ("time_window", None, KW), ("random_seed", None, KW),
        ("need_center_local_output", False, KW), ("need_edge_output", False, KW)]
    sig = inspect.signature(wgth.GraphStructure.multilayer_temporal_sample)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("node_ids", E, POS), ("node_times", E, POS), ("max_neighbors", E, POS), ("time_name", E, POS), ("strategy", "uniform", KW),
        ("inclusive", True, KW), ("time_window", None, KW), ("propagate", "seed", KW), ("random_seeds", None, KW),
        ("edge_attr_names", None, KW)]
    assert [p.name for p in inspect.signature(temporal.TimeEncoder.__init__).parameters.values()] == ["self", "dim"]
    sig = inspect.signature(temporal.TemporalGNNModel.__init__)
    assert [p.name for p in sig.parameters.values()] == ["self", "graph_structure", "node_embedding", "args", "time_name"]
    assert [p.name for p in inspect.signature(temporal.TemporalGNNModel.forward).parameters.values()][:3] == ["self", "seeds", "seed_times"]
    assert wgth.wholegraph_ops.temporal_sample_without_replacement is wholegraph_ops.temporal_sample_without_replacement
    assert alias.wholegraph_ops.temporal_sample_without_replacement is wholegraph_ops.temporal_sample_without_replacement
    assert alias.GraphStructure.temporal_sample_one_hop is wgth.GraphStructure.temporal_sample_one_hop
    assert alias.GraphStructure.multilayer_temporal_sample is wgth.GraphStructure.multilayer_temporal_sample
    assert wgth.TimeEncoder is temporal.TimeEncoder and alias.TimeEncoder is temporal.TimeEncoder
    assert wgth.TemporalGNNModel is temporal.TemporalGNNModel and alias.TemporalGNNModel is temporal.TemporalGNNModel
    assert alias.temporal is temporal and {"TimeEncoder", "TemporalGNNModel", "temporal"} <= set(wgth.__all__)


def test_time_encoder_is_tgats():
    import torch
    from wholegraph_amd.torch.temporal import TimeEncoder
    enc = TimeEncoder(10)
    w = (10.0 ** -torch.linspace(0, 9, 10, dtype=torch.float64)).to(torch.float32)
    assert torch.equal(enc.lin.weight.detach().reshape(-1), w) and torch.equal(enc.lin.bias.detach(), torch.zeros(10))
    dt = torch.tensor([0, 1, 1000, 123456789], dtype=torch.int64)
    out = enc(dt)
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 10) and torch.equal(out[0], torch.ones(10))
    assert torch.allclose(out, torch.cos(dt.to(torch.float32).unsqueeze(1) * w.unsqueeze(0)), atol=1e-6)
    assert {n for n, p in enc.named_parameters() if p.requires_grad} == {"lin.weight", "lin.bias"}


def test_python_side_errors_come_before_the_library(wm_lib, monkeypatch):
    import types
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    from wholegraph_amd.torch import wholegraph_ops
    monkeypatch.setattr(binding, "lib", lambda: pytest.fail("reached the library"))
    nodes, times = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    sample = wholegraph_ops.temporal_sample_without_replacement
    with pytest.raises(ValueError, match="strategy"):
        sample(None, None, None, nodes, times, 5, strategy="first")
    with pytest.raises(ValueError, match="at most 64"):
        sample(None, None, None, nodes, times, 65)
    for window in (-1, 1 << 63):
        with pytest.raises(ValueError, match="time_window"):
            sample(None, None, None, nodes, times, 5, time_window=window)
    for bad_nodes, bad_times in ((nodes.reshape(2, 2), times), (nodes, times.reshape(2, 2)), (nodes[0], times[0])):
        with pytest.raises(ValueError, match="1-D"):
            sample(None, None, None, bad_nodes, bad_times, 5)
    with pytest.raises(ValueError, match="one time per centre"):
        sample(None, None, None, nodes, times[:3], 5)
    with pytest.raises(ValueError, match="int64"):
        sample(None, None, None, nodes, times.to(torch.int32), 5)
    g = wgth.GraphStructure()
    g.csr_row_ptr = g.csr_col_ind = types.SimpleNamespace(wmb_tensor=None)
    with pytest.raises(AssertionError, match="no edge attribute named"):
        g.temporal_sample_one_hop("missing", nodes, times, 5)
    g.edge_attributes["t32"] = types.SimpleNamespace(wmb_tensor=None, dtype=torch.int32, dim=lambda: 1)
    g.edge_attributes["t"] = types.SimpleNamespace(wmb_tensor=None, dtype=torch.int64, dim=lambda: 1)
    with pytest.raises(AssertionError, match="int64 timestamps"):
        g.temporal_sample_one_hop("t32", nodes, times, 5)
    with pytest.raises(ValueError, match="at most 64"):
        g.temporal_sample_one_hop("t", nodes, times, 100)
    with pytest.raises(ValueError, match="propagate"):
        g.multilayer_temporal_sample(nodes, times, [5, 5], "t", propagate="node")
    with pytest.raises(AssertionError, match="one seed per hop"):
        g.multilayer_temporal_sample(nodes, times, [5, 5], "t", random_seeds=[1])
    with pytest.raises(AssertionError, match="no edge attribute named"):
        g.multilayer_temporal_sample(nodes, times, [5, 5], "t", edge_attr_names=["missing"])
    with pytest.raises(ValueError, match="strategy"):
        g.multilayer_temporal_sample(nodes, times, [5, 5], "t", strategy="first")


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
      np.dtype(np.int16): wmb.DT_INT16, np.dtype(np.float64): wmb.DT_DOUBLE}
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
i64, i32, f32, f64, i16 = np.int64, np.int32, np.float32, np.float64, np.int16
env = wmb.EnvFunc()          # (never called: every answer here comes before the first allocation)
ctx = C.c_void_p(1)          # (a memory context is opaque to the library and only handed to the env functions)
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), time=wrap(np.zeros(n_edges, i64)),
          nodes=wrap(np.zeros(n, i64)), times=wrap(np.zeros(n, i64)), m=5, strategy=0, inclusive=1, window=-1,
          off=wrap(np.zeros(n + 1, i32)), dctx=ctx, lctx=None, ectx=None, env=C.byref(env))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_temporal_sample(a["row"], a["col"], a["time"], a["nodes"], a["times"], a["m"], a["strategy"],
                                                 a["inclusive"], a["window"], 77, a["off"], a["dctx"], a["lctx"], a["ectx"],
                                                 a["env"], None)
huge = (1 << 31) - 1      # (a description of 2^31 - 1 centres over a one-entry array: refused before anything is read)
row32, colf, nodesf, off64 = wrap(np.zeros(n_nodes + 1, i32)), wrap(np.zeros(n_edges, f32)), wrap(np.zeros(n, f32)), wrap(np.zeros(n + 1, i64))
time32, times32 = wrap(np.zeros(n_edges, i32)), wrap(np.zeros(n, i32))
invalid = [call(row=None), call(col=None), call(time=None), call(nodes=None), call(times=None), call(off=None), call(dctx=None),
           call(env=None),
           call(row=wrap(np.zeros((2, 3), i64))), call(col=wrap(np.zeros((7, 1), i64))), call(time=wrap(np.zeros((7, 1), i64))),
           call(nodes=wrap(np.zeros((2, 2), i64))), call(times=wrap(np.zeros((2, 2), i64))), call(off=wrap(np.zeros((n + 1, 1), i32))),
           call(m=65), call(m=1 << 20), call(strategy=2), call(strategy=-1),
           call(time=wrap(np.zeros(n_edges - 1, i64))), call(time=wrap(np.zeros(n_edges + 1, i64))),      # not one entry per edge
           call(times=wrap(np.zeros(n - 1, i64))), call(times=wrap(np.zeros(n + 1, i64))),                 # not n entries
           call(nodes=wrap(np.zeros(1, i64), [huge]), times=wrap(np.zeros(1, i64), [huge]), off=wrap(np.zeros(1, i32), [huge + 1])),
           call(off=wrap(np.zeros(n, i32))), call(off=wrap(np.zeros(0, i32))),                             # shorter than n + 1
           # two faults, one of shape, size or scalar and one of dtype: the former's answer
           call(m=65, row=row32), call(strategy=2, time=time32), call(time=wrap(np.zeros(n_edges - 1, i32))),
           call(times=wrap(np.zeros(n - 1, i32))), call(nodes=wrap(np.zeros((2, 2), i64)), row=row32), call(dctx=None, col=colf),
           call(env=None, nodes=nodesf), call(off=wrap(np.zeros(n, i64))), call(off=wrap(np.zeros(n, i32)), times=times32),
           call(col=wrap(np.zeros((7, 1), f32))), call(row=None, off=off64)]
logic = [call(row=row32), call(row=wrap(np.zeros(n_nodes + 1, f32))), call(col=colf), call(col=wrap(np.zeros(n_edges, i16))),
         call(nodes=nodesf), call(nodes=wrap(np.zeros(n, i16))), call(time=time32), call(time=wrap(np.zeros(n_edges, f64))),
         call(times=times32), call(times=wrap(np.zeros(n, f64))), call(off=off64), call(off=wrap(np.zeros(n + 1, f32))),
         # two dtype faults; and a dtype fault with the optional contexts given
         call(row=row32, off=off64), call(time=time32, times=times32), call(col=colf, nodes=nodesf),
         call(off=off64, lctx=ctx, ectx=ctx)]
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [call(), call(lctx=ctx, ectx=ctx), call(nodes=wrap(np.zeros(n, i32))), call(col=wrap(np.zeros(n_edges, i32))),
            call(m=64, strategy=1, inclusive=0, window=50), call(m=0), call(m=-1), call(off=wrap(np.zeros(n + 9, i32))),
            call(col=wrap(np.zeros(0, i64)), time=wrap(np.zeros(0, i64))),
            call(nodes=wrap(np.zeros(0, i64)), times=wrap(np.zeros(0, i64)), off=wrap(np.zeros(1, i32)))]
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
    assert len(invalid) == 36 and invalid == [INV] * 36        # (the argument checks come first, whatever the backend)
    assert len(logic) == 16 and logic == [LOGIC] * 16
    assert good == [binding.NOT_SUPPORTED] * 10                 # no such kernels in that backend: nothing queued


def test_argument_checks_under_the_product_backend(wm_lib):
    """the same malformed calls with the product's backend installed and no device: answered before any device work"""
    invalid, logic, good = _child("hip")
    assert invalid == [INV] * 36 and logic == [LOGIC] * 16 and good == []
