"""The surface of `gather_agg_concat` over an 8-bit row-quantized table (header section 2j) without a GPU: exported names,
the header's order, unchanged signatures, the argument checks of the C entry point (they come before the backend is looked
at, so they hold under every backend), the entry point under the CPU test backend (no such kernel there: NOT_SUPPORTED, the
counter stays 0), and what the Python function refuses."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wholememory_ext_csc_gather_dequantize_aggregate_forward", "wholememory_ext_gather_dequantize_aggregate_calls")


def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    from wholegraph_amd.torch import gather_aggregation
    assert callable(gather_aggregation.quantized_calls) and callable(gather_aggregation.takes_fused_route)
    for name in NEW:
        assert hasattr(wm_lib, name), name
        assert name in binding.PROTOTYPES, name
    restype, argtypes = binding.PROTOTYPES[NEW[0]]
    assert restype is C.c_int and len(argtypes) == 14
    assert binding.PROTOTYPES[NEW[1]] == (C.c_int64, [])
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    for name in NEW:
        assert name in header
    assert isinstance(wm_lib.wholememory_ext_gather_dequantize_aggregate_calls(), int)
    assert wgth.gather_agg_concat is gather_aggregation.gather_agg_concat


def test_header_order():
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    contents, body = header.split("#ifndef WHOLEMEMORY_WHOLEGRAPH_AMD_EXT_H_")
    # the contents at the top: one line per section
    assert contents.index("(2i) 8-bit row-quantized") < contents.index("(2j) ") < contents.index("(3) the testing seam")
    # the blocks
    marks = [body.index("/* ---- (2i) "), body.index("/* ---- (2j) "), body.index("/* ---- (3) testing seam")]
    assert marks == sorted(marks) and body.count("/* ---- (2j) ") == 1
    block = body[marks[1]:marks[2]]
    for name in NEW:
        assert name in block and name not in body[:marks[1]]


def test_signatures_are_unchanged(wm_lib):
    import wholegraph_amd.torch as wgth
    sig = inspect.signature(wgth.gather_agg_concat)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("source", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("node_ids", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("csr_row_ptr", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("csr_col_ind", inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("aggr", "mean", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("is_training", False, inspect.Parameter.KEYWORD_ONLY)]
    sig = inspect.signature(wgth.cugraphops.CuGraphSAGEConv.forward_from_table)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("source", inspect.Parameter.empty), ("node_ids", inspect.Parameter.empty),
        ("csr_row_ptr", inspect.Parameter.empty), ("csr_col_ind", inspect.Parameter.empty),
        ("max_num_neighbors", inspect.Parameter.empty), ("is_training", False)]
    assert "WholeMemoryQuantizedTensor" in wgth.cugraphops.CuGraphSAGEConv.forward_from_table.__doc__
    assert list(inspect.signature(wgth.HomoGNNModel.__init__).parameters) == ["self", "graph_structure", "node_embedding", "args"]


def _table(L, wmb, buf, sizes, dtype, strides=None, offset=0):
    desc = wmb.make_tensor_desc(list(sizes), dtype, strides, offset)
    t = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(t), C.cast(buf, C.c_void_p), C.byref(desc)))
    return t


def test_entry_point_validates_arguments(wm_lib):
    """every check of section 2j, through handle-less tensors: INVALID_INPUT before the backend is looked at"""
    from wholegraph_amd import binding as wmb
    L = wm_lib
    F, N = 6, 5                    # Q = 8, row_bytes = 16
    RB = 16
    assert L.wholememory_ext_quantized_row_bytes(F) == RB
    buf = (C.c_char * 4096)()
    out = (C.c_float * 256)()
    ids = (C.c_int64 * 3)(0, 1, 2)
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(2, 0)
    env = L.wholememory_get_default_env_func()
    tables = {"ok": _table(L, wmb, buf, (N, RB), wmb.DT_INT8),
              "one_d": _table(L, wmb, buf, (N * RB,), wmb.DT_INT8),
              "three_d": _table(L, wmb, buf, (N, 1, RB), wmb.DT_INT8),
              "float": _table(L, wmb, buf, (N, RB), wmb.DT_FLOAT),
              "int": _table(L, wmb, buf, (N, RB), wmb.DT_INT),
              "short_rows": _table(L, wmb, buf, (N, RB - 1), wmb.DT_INT8, [RB, 1]),
              "codes_only": _table(L, wmb, buf, (N, 8), wmb.DT_INT8, [RB, 1]),
              "stride_18": _table(L, wmb, buf, (N, RB), wmb.DT_INT8, [RB + 2, 1]),
              "stride_below_row": _table(L, wmb, buf, (N, RB), wmb.DT_INT8, [RB - 4, 1]),
              "offset_2": _table(L, wmb, buf, (N, RB), wmb.DT_INT8, [RB, 1], 2),
              "no_rows": _table(L, wmb, buf, (0, RB), wmb.DT_INT8, [RB, 1])}
    ok = dict(table=tables["ok"], dim=F, ids=ids, idt=wmb.DT_INT64, row_ptr=rp, col=col, E=2, nd=2, ns=3, aggr=wmb.AGGR_MEAN,
              out=out, os=2 * F)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gather_dequantize_aggregate_forward(
            a["table"], a["dim"], a["ids"], a["idt"], a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["aggr"], a["out"],
            a["os"], env, None)

    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    before = L.wholememory_ext_gather_dequantize_aggregate_calls()
    # (an inner stride other than 1 is refused where the tensor is made: no such table reaches the entry point's own check)
    desc = wmb.make_tensor_desc([N, RB], wmb.DT_INT8, [2 * RB, 2], 0)
    assert L.wholememory_make_tensor_from_pointer(C.byref(C.c_void_p()), C.cast(buf, C.c_void_p), C.byref(desc)) == inv
    try:
        # the table and its width
        for bad in (dict(table=None), dict(table=tables["one_d"]), dict(table=tables["three_d"]), dict(table=tables["float"]),
                    dict(table=tables["int"]), dict(dim=0), dict(dim=-4),
                    dict(table=tables["short_rows"]), dict(table=tables["codes_only"]), dict(dim=9), dict(dim=RB),
                    dict(table=tables["stride_18"]), dict(table=tables["stride_below_row"]), dict(table=tables["offset_2"])):
            assert fwd(**bad) == inv, bad
        # the ids' type
        for bad in (dict(idt=wmb.DT_FLOAT), dict(idt=wmb.DT_INT16), dict(idt=wmb.DT_INT8), dict(idt=0)):
            assert fwd(**bad) == inv, bad
        # the block, as agg_concat's entry points judge it
        for bad in (dict(row_ptr=None), dict(col=None), dict(ids=None), dict(out=None), dict(E=-1), dict(nd=-1), dict(ns=-1),
                    dict(nd=4), dict(os=2 * F - 1), dict(os=F), dict(aggr=7), dict(aggr=-1), dict(E=1 << 31)):
            assert fwd(**bad) == inv, bad
        # node ids into a table without rows
        assert fwd(table=tables["no_rows"]) == inv
        assert L.wholememory_ext_gather_dequantize_aggregate_calls() == before
    finally:
        for t in tables.values():
            L.wholememory_destroy_tensor(t)


_CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
os.environ["WHOLEGRAPH_AMD_TESTING"] = "1"
from wholegraph_amd import binding as wmb
L = wmb.lib()
tb = C.CDLL(os.path.join(sys.argv[1], "oracle", "libwm_test_backend.so"))
tb.wm_test_backend.restype = C.c_void_p
wmb.check(L.wm_testing_install_backend(C.c_void_p(tb.wm_test_backend())))
assert L.wholememory_ext_backend_name().startswith(b"oracle-test-backend")
F, N, RB = 6, 5, 16
buf = (C.c_char * (N * RB))()
desc = wmb.make_tensor_desc([N, RB], wmb.DT_INT8, None, 0)
t = C.c_void_p()
wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(t), C.cast(buf, C.c_void_p), C.byref(desc)))
ids = (C.c_int64 * 3)(0, 1, 2)
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
out = (C.c_float * (2 * 2 * F))()
env = L.wholememory_get_default_env_func()
before = L.wholememory_ext_gather_dequantize_aggregate_calls()
fwd = L.wholememory_ext_csc_gather_dequantize_aggregate_forward(t, F, ids, wmb.DT_INT64, row_ptr, col, 2, 2, 3, wmb.AGGR_MEAN,
                                                                out, 2 * F, env, None)
# a malformed call is still INVALID_INPUT under this backend
bad = L.wholememory_ext_csc_gather_dequantize_aggregate_forward(t, F, ids, wmb.DT_INT64, row_ptr, col, 2, 2, 3, wmb.AGGR_MEAN,
                                                                out, 2 * F - 1, env, None)
print("RESULT", fwd, bad, before, L.wholememory_ext_gather_dequantize_aggregate_calls(), int(any(out)))
'''


def test_entry_point_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    fwd, bad, before, after, written = (int(v) for v in line.split()[1:])
    from wholegraph_amd import binding
    assert fwd == binding.NOT_SUPPORTED and bad == 6
    assert before == 0 and after == 0 and written == 0


def test_python_refusals(wm_lib):
    """what gather_agg_concat refuses before it looks at a table's memory: the aggregators first, then the source's type,
    then the shape and type of the ids"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.quantized import WholeMemoryQuantizedTensor
    ids = torch.zeros(2, dtype=torch.int64)
    rp = torch.tensor([0, 1], dtype=torch.int32)
    ci = torch.tensor([1], dtype=torch.int32)
    q = WholeMemoryQuantizedTensor.__new__(WholeMemoryQuantizedTensor)   # (never dereferenced: refused before that)
    q.storage, q.dim_ = None, 8
    for source in (object(), q):
        for aggr in ("max", "min"):
            with pytest.raises(NotImplementedError):
                wgth.gather_agg_concat(source, ids, rp, ci, aggr)
        with pytest.raises(ValueError):
            wgth.gather_agg_concat(source, ids, rp, ci, "median")
    with pytest.raises(TypeError):
        wgth.gather_agg_concat(object(), ids, rp, ci, "mean")
    with pytest.raises(ValueError, match="1-D"):
        wgth.gather_agg_concat(q, ids.reshape(1, 2), rp, ci, "mean")
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int16)):
        with pytest.raises(TypeError, match="int32 or int64"):
            wgth.gather_agg_concat(q, bad, rp, ci, "mean")
    with pytest.raises(ValueError, match="more targets"):
        wgth.gather_agg_concat(q, ids, torch.tensor([0, 1, 1, 1], dtype=torch.int32), ci, "mean")   # 3 targets, 2 ids
