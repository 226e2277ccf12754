"""The surface of `gather_agg_concat` (agg_concat straight from a WholeMemory table) without a GPU: exported names and
signatures, the layer method that refuses project=True, the argument checks of the C entry point (they come before any
device work), the entry points under the CPU test backend (no such kernel there: NOT_SUPPORTED, the counter stays 0), and the
aggregators that are still refused."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wholememory_ext_csc_gather_aggregate_forward", "wholememory_ext_gather_aggregate_calls")


def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    assert wgth.gather_aggregation is gather_aggregation and "gather_aggregation" in wgth.__all__
    assert wgth.gather_agg_concat is gather_aggregation.gather_agg_concat and "gather_agg_concat" in wgth.__all__
    assert callable(gather_aggregation.calls) and callable(gather_aggregation.takes_fused_route)
    for name in NEW:
        assert hasattr(wm_lib, name), name
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    for name in NEW:
        assert name in header
    assert header.index("(2d)") < header.index("(2e)") < header.index("(3) testing seam")
    assert isinstance(wm_lib.wholememory_ext_gather_aggregate_calls(), int)


def test_signatures(wm_lib):
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
    # forward and __init__ keep the reference's signatures
    assert list(inspect.signature(wgth.cugraphops.CuGraphSAGEConv.forward).parameters) == [
        "self", "x", "csr_row_ptr", "csr_col_ind", "max_num_neighbors"]


def test_forward_from_table_refuses_project(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    layer = wgth.cugraphops.CuGraphSAGEConv(8, 4, project=True)
    ids = torch.zeros(2, dtype=torch.int64)
    rp = torch.tensor([0, 1], dtype=torch.int32)
    ci = torch.tensor([1], dtype=torch.int32)
    with pytest.raises(ValueError, match="project"):
        layer.forward_from_table(object(), ids, rp, ci, 4)   # (refused before the source is looked at)


def test_max_min_still_refused_and_bad_sources(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    ids = torch.zeros(2, dtype=torch.int64)
    rp = torch.tensor([0, 1], dtype=torch.int32)
    ci = torch.tensor([1], dtype=torch.int32)
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError):
            wgth.gather_agg_concat(object(), ids, rp, ci, aggr)
        with pytest.raises(NotImplementedError):
            wgth.cugraphops.CuGraphSAGEConv(8, 4, aggr=aggr)
    with pytest.raises(ValueError):
        wgth.gather_agg_concat(object(), ids, rp, ci, "median")
    with pytest.raises(TypeError):
        wgth.gather_agg_concat(object(), ids, rp, ci, "mean")   # neither an embedding nor a WholeMemory tensor


def test_model_reads_the_flag_and_defaults_to_off(wm_lib):
    from wholegraph_amd.torch import gnn_model
    src = inspect.getsource(gnn_model.HomoGNNModel)
    assert 'getattr(args, "fuse_gather", False)' in src and "forward_from_table" in src


def _table(L, wmb, buf, sizes, dtype, strides=None):
    desc = wmb.make_tensor_desc(list(sizes), dtype, strides, 0)
    t = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(t), C.cast(buf, C.c_void_p), C.byref(desc)))
    return t


def test_entry_point_validates_arguments(wm_lib):
    """argument checks that come before any device work (the installed backend here is the product's: the calls are
    rejected before they could touch memory)"""
    from wholegraph_amd import binding as wmb
    L = wm_lib
    F, N = 4, 5
    buf = (C.c_float * 256)()
    ids = (C.c_int64 * 3)(0, 1, 2)
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(2, 0)
    env = L.wholememory_get_default_env_func()
    tables = {"ok": _table(L, wmb, buf, (N, F), wmb.DT_FLOAT),
              "one_d": _table(L, wmb, buf, (N * F,), wmb.DT_FLOAT),
              "int": _table(L, wmb, buf, (N, F), wmb.DT_INT),
              "int64": _table(L, wmb, buf, (N, F), wmb.DT_INT64),
              "double": _table(L, wmb, buf, (N, F), wmb.DT_DOUBLE),
              "no_columns": _table(L, wmb, buf, (N, 0), wmb.DT_FLOAT, [4, 1])}
    ok = dict(table=tables["ok"], ids=ids, idt=wmb.DT_INT64, row_ptr=rp, col=col, E=2, nd=2, ns=3, aggr=wmb.AGGR_MEAN,
              out=buf, os=2 * F)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gather_aggregate_forward(a["table"], a["ids"], a["idt"], a["row_ptr"], a["col"], a["E"],
                                                              a["nd"], a["ns"], a["aggr"], a["out"], a["os"], env, None)

    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    try:
        # what the agg_concat entry points reject ...
        for bad in (dict(row_ptr=None), dict(col=None), dict(ids=None), dict(out=None), dict(E=-1), dict(nd=-1), dict(ns=-1),
                    dict(nd=4), dict(aggr=7), dict(aggr=-1), dict(table=tables["no_columns"]), dict(E=1 << 31)):
            assert fwd(**bad) == inv, bad
        # ... plus what is new here
        for bad in (dict(table=None), dict(table=tables["one_d"]), dict(table=tables["int"]), dict(table=tables["int64"]),
                    dict(table=tables["double"]), dict(idt=wmb.DT_FLOAT), dict(idt=wmb.DT_INT16), dict(idt=0),
                    dict(os=2 * F - 1), dict(os=F)):
            assert fwd(**bad) == inv, bad
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
F, N = 4, 5
buf = (C.c_float * (N * F))()
desc = wmb.make_tensor_desc([N, F], wmb.DT_FLOAT, None, 0)
t = C.c_void_p()
wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(t), C.cast(buf, C.c_void_p), C.byref(desc)))
ids = (C.c_int64 * 3)(0, 1, 2)
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
out = (C.c_float * (2 * 2 * F))()
env = L.wholememory_get_default_env_func()
before = L.wholememory_ext_gather_aggregate_calls()
fwd = L.wholememory_ext_csc_gather_aggregate_forward(t, ids, wmb.DT_INT64, row_ptr, col, 2, 2, 3, wmb.AGGR_MEAN, out, 2 * F,
                                                     env, None)
print("RESULT", fwd, before, L.wholememory_ext_gather_aggregate_calls())
# a malformed call is judged before the backend is asked (the op has a forward only): a null row_ptr, an out stride one
# short of the row
bad_ptr = L.wholememory_ext_csc_gather_aggregate_forward(t, ids, wmb.DT_INT64, None, col, 2, 2, 3, wmb.AGGR_MEAN, out, 2 * F,
                                                         env, None)
bad_stride = L.wholememory_ext_csc_gather_aggregate_forward(t, ids, wmb.DT_INT64, row_ptr, col, 2, 2, 3, wmb.AGGR_MEAN, out,
                                                            2 * F - 1, env, None)
print("MALFORMED", bad_ptr, bad_stride)
'''


def test_entry_points_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    fwd, before, after = (int(v) for v in line.split()[1:])
    from wholegraph_amd import binding
    assert fwd == binding.NOT_SUPPORTED
    assert before == 0 and after == 0
    malformed = [l for l in p.stdout.splitlines() if l.startswith("MALFORMED")][-1]
    assert [int(v) for v in malformed.split()[1:]] == [6, 6]   # WHOLEMEMORY_INVALID_INPUT
