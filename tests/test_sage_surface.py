"""The GraphSAGE / GNN-model surface without a GPU: names and signatures of the reference's cugraph route, framework
selection, and the aggregation entry points under the CPU test backend (which has no such kernels: NOT_SUPPORTED, no
crash)."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gnn_model
    for name in ("set_framework", "create_gnn_layers", "create_sub_graph", "HomoGNNModel"):
        assert getattr(wgth, name) is getattr(gnn_model, name)
        assert name in wgth.__all__
    from wholegraph_amd.torch.cugraphops.sage_conv import CuGraphSAGEConv
    assert wgth.cugraphops.CuGraphSAGEConv is CuGraphSAGEConv
    assert callable(gnn_model.layer_forward) and callable(gnn_model.parse_max_neighbors)


def test_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    sig = inspect.signature(wgth.cugraphops.CuGraphSAGEConv.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty), ("aggr", "mean"),
        ("normalize", False), ("root_weight", True), ("project", False), ("bias", True)]
    fwd = inspect.signature(wgth.cugraphops.CuGraphSAGEConv.forward)
    assert list(fwd.parameters) == ["self", "x", "csr_row_ptr", "csr_col_ind", "max_num_neighbors"]
    assert list(inspect.signature(wgth.HomoGNNModel.__init__).parameters) == ["self", "graph_structure", "node_embedding",
                                                                              "args"]
    assert list(inspect.signature(wgth.HomoGNNModel.forward).parameters) == ["self", "ids"]
    assert list(inspect.signature(wgth.create_gnn_layers).parameters) == [
        "in_feat_dim", "hidden_feat_dim", "class_count", "num_layer", "num_head", "model_type"]
    assert list(inspect.signature(wgth.create_sub_graph).parameters) == [
        "target_gid", "target_gid_1", "edge_data", "csr_row_ptr", "csr_col_ind", "max_num_neighbors", "add_self_loop"]


def test_set_framework_and_layers(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gnn_model
    for bad in ("dgl", "pyg", "wg", "tensorflow"):
        with pytest.raises(ValueError, match="cugraph"):
            wgth.set_framework(bad)
    wgth.set_framework("cugraph")
    layers = wgth.create_gnn_layers(32, 64, 5, 3, 1, "sage")
    assert [(l.in_channels, l.out_channels) for l in layers] == [(32, 64), (64, 64), (64, 5)]
    assert all(isinstance(l, wgth.cugraphops.CuGraphSAGEConv) for l in layers)
    with pytest.raises(NotImplementedError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gat")
    assert gnn_model.parse_max_neighbors(3, "15") == [15, 15, 15]
    assert gnn_model.parse_max_neighbors(2, "30,20") == [30, 20]
    sub = wgth.create_sub_graph(None, None, None, "row", "col", 10, False)
    assert sub == ["row", "col", 10]


def test_sage_conv_parameters_and_aggr(wm_lib):
    from wholegraph_amd.torch.aggregation import aggr_code
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    layer = CuGraphSAGEConv(16, 8)
    assert tuple(layer.lin.weight.shape) == (8, 32) and layer.lin.bias is not None
    layer = CuGraphSAGEConv(16, 8, root_weight=False, project=True, bias=False)
    assert tuple(layer.lin.weight.shape) == (8, 16) and layer.lin.bias is None
    assert tuple(layer.pre_lin.weight.shape) == (16, 16)
    with pytest.raises(NotImplementedError):
        CuGraphSAGEConv(16, 8, aggr="max")
    with pytest.raises(ValueError):
        CuGraphSAGEConv(16, 8, aggr="avg")
    assert aggr_code("sum") == 0 and aggr_code("mean") == 1


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
F, nd, ns = 4, 2, 3
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
x = (C.c_float * (ns * F))()
out = (C.c_float * (nd * 2 * F))()
gx = (C.c_float * (ns * F))()
env = L.wholememory_get_default_env_func()
fwd = L.wholememory_ext_csc_aggregate_forward(row_ptr, col, 2, nd, ns, x, F, F, wmb.AGGR_MEAN, out, 2 * F, env, None)
bwd = L.wholememory_ext_csc_aggregate_backward(row_ptr, col, 2, nd, ns, out, 2 * F, F, wmb.AGGR_SUM, gx, F, env, None)
print("RESULT", fwd, bwd, L.wholememory_ext_csc_aggregate_chunk_edges())
# a malformed call is judged before the backend is asked: a null row_ptr, a grad_x stride one short of the row
bad_fwd = L.wholememory_ext_csc_aggregate_forward(None, col, 2, nd, ns, x, F, F, wmb.AGGR_MEAN, out, 2 * F, env, None)
bad_bwd = L.wholememory_ext_csc_aggregate_backward(row_ptr, col, 2, nd, ns, out, 2 * F, F, wmb.AGGR_SUM, gx, F - 1, env, None)
print("MALFORMED", bad_fwd, bad_bwd)
'''


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    fwd, bwd, chunk = (int(v) for v in line.split()[1:])
    from wholegraph_amd import binding
    assert fwd == binding.NOT_SUPPORTED and bwd == binding.NOT_SUPPORTED
    assert chunk >= 1
    malformed = [l for l in p.stdout.splitlines() if l.startswith("MALFORMED")][-1]
    assert [int(v) for v in malformed.split()[1:]] == [6, 6]   # WHOLEMEMORY_INVALID_INPUT


def test_entry_points_validate_arguments(wm_lib):
    """argument checks that come before any device work (the installed backend here is the product's: the calls are
    rejected before they could touch memory)"""
    import ctypes as C
    from wholegraph_amd import binding
    L = wm_lib
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 64)()
    env = L.wholememory_get_default_env_func()
    ok = dict(row_ptr=rp, col=col, E=2, nd=2, ns=3, x=buf, xs=4, dim=4, aggr=binding.AGGR_MEAN, out=buf, os=8)

    def call(fn, **over):
        a = dict(ok, **over)
        return fn(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["x"], a["xs"], a["dim"], a["aggr"], a["out"], a["os"],
                  env, None)

    fwd, bwd = L.wholememory_ext_csc_aggregate_forward, L.wholememory_ext_csc_aggregate_backward
    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    for fn in (fwd, bwd):
        assert call(fn, row_ptr=None) == inv
        assert call(fn, col=None) == inv
        assert call(fn, x=None) == inv
        assert call(fn, out=None) == inv
        assert call(fn, E=-1) == inv
        assert call(fn, nd=-1) == inv
        assert call(fn, ns=-1) == inv
        assert call(fn, nd=4) == inv           # more targets than rows of x
        assert call(fn, dim=0) == inv
        assert call(fn, aggr=7) == inv
    assert call(fwd, xs=3) == inv               # x rows of 4 floats
    assert call(fwd, os=7) == inv               # out rows of 8 floats
    assert call(bwd, xs=7) == inv               # grad_out rows of 8 floats
    assert call(bwd, os=3) == inv               # grad_x rows of 4 floats
