"""The relation-typed aggregation surface without a GPU: the two C entry points (exported, bound, stated in the header in
section (2h) between (2g) and the testing seam), NOT_SUPPORTED under the CPU test backend (which has no such kernels) and
the argument checks that come before any device work; names, signatures and parameter shapes of agg_concat_rel, RGCNConv
and create_rgcn_layers, the Python-side errors, and the model name "rgcn"."""
import inspect
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 6   # WHOLEMEMORY_INVALID_INPUT
FWD = "wholememory_ext_csc_rel_aggregate_forward"
BWD = "wholememory_ext_csc_rel_aggregate_backward"


def test_symbols_exported_and_bound(wm_lib):
    from wholegraph_amd import binding
    fwd, bwd = binding.PROTOTYPES[FWD], binding.PROTOTYPES[BWD]
    assert len(fwd[1]) == 16 and len(bwd[1]) == 16
    assert hasattr(wm_lib, FWD) and hasattr(wm_lib, BWD)


def test_header_states_the_op_between_2g_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    f2, g2, h2, seam = (text.index("---- (2f)"), text.index("---- (2g)"), text.index("---- (2h)"),
                        text.index("---- (3) testing seam"))
    assert f2 < g2 < h2 < seam
    head = text[:text.index("#ifndef")]
    assert "(2h)" in head and head.index("(2g)") < head.index("(2h)") < head.index("(3) the testing seam")
    for name in (FWD, BWD):
        assert h2 < text.index(name + "(") < seam


def test_exported_names_and_signatures(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gnn_model, rel_aggregation
    from wholegraph_amd.torch.cugraphops.rgcn_conv import RGCNConv
    assert wgth.cugraphops.RGCNConv is RGCNConv and "RGCNConv" in wgth.cugraphops.__all__
    assert wgth.cugraphops.__all__[-1] == "EdgeWeightedSAGEConv"
    assert wgth.cugraphops.__all__[:2] == ["CuGraphSAGEConv", "CuGraphGATConv"]
    assert "rel_aggregation" in wgth.__all__ and wgth.rel_aggregation is rel_aggregation
    assert issubclass(rel_aggregation.CscAggregateConcatRel, torch.autograd.Function)
    import pylibwholegraph.torch as pwt
    assert pwt.cugraphops.RGCNConv is RGCNConv and pwt.rel_aggregation is rel_aggregation
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(rel_aggregation.agg_concat_rel).parameters.values()] == [
        ("x", E), ("csr_row_ptr", E), ("csr_col_ind", E), ("edge_type", E), ("num_relations", E), ("aggr", "mean")]
    assert [(p.name, p.default) for p in list(inspect.signature(RGCNConv.__init__).parameters.values())[1:]] == [
        ("in_channels", E), ("out_channels", E), ("num_relations", E), ("num_bases", None), ("aggr", "mean"),
        ("root_weight", True), ("bias", True)]
    assert list(inspect.signature(RGCNConv.forward).parameters) == [
        "self", "x", "csr_row_ptr", "csr_col_ind", "max_num_neighbors", "edge_type"]
    assert [(p.name, p.default) for p in inspect.signature(gnn_model.create_rgcn_layers).parameters.values()] == [
        ("in_feat_dim", E), ("hidden_feat_dim", E), ("class_count", E), ("num_layer", E), ("num_relations", E),
        ("num_bases", None)]
    # the pinned signatures are the ones they were
    assert list(inspect.signature(wgth.create_gnn_layers).parameters) == [
        "in_feat_dim", "hidden_feat_dim", "class_count", "num_layer", "num_head", "model_type"]
    assert list(inspect.signature(wgth.HomoGNNModel.forward).parameters) == ["self", "ids"]
    assert list(inspect.signature(wgth.HomoGNNModel.__init__).parameters) == [
        "self", "graph_structure", "node_embedding", "args"]
    doc = RGCNConv.__doc__
    assert "out of scope" in doc and "agg_hg_basis_n2n_post" in doc and 'aggr="sum"' in doc and "TOTAL degree" in doc


@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("num_bases", [None, 2])
def test_parameter_shapes(wm_lib, root_weight, bias, num_bases):
    from wholegraph_amd.torch.cugraphops import RGCNConv
    layer = RGCNConv(16, 8, 5, num_bases=num_bases, root_weight=root_weight, bias=bias)
    assert tuple(layer.weight.shape) == ((5, 16, 8) if num_bases is None else (2, 16, 8)) and layer.weight.abs().sum() > 0
    if num_bases is None:
        assert layer.comp is None
    else:
        assert tuple(layer.comp.shape) == (5, 2) and layer.comp.abs().sum() > 0
    if root_weight:
        assert tuple(layer.root.shape) == (16, 8) and layer.root.abs().sum() > 0
    else:
        assert layer.root is None
    if bias:
        assert tuple(layer.bias.shape) == (8,) and not layer.bias.any()
    else:
        assert layer.bias is None
    names = sorted(n for n, _ in layer.named_parameters())
    want = ["weight"] + (["comp"] if num_bases else []) + (["root"] if root_weight else []) + (["bias"] if bias else [])
    assert names == sorted(want)
    layer.reset_parameters()
    assert (layer.in_channels, layer.out_channels, layer.num_relations, layer.num_bases, layer.aggr) == (
        16, 8, 5, num_bases, "mean")
    assert repr(layer) == "RGCNConv(16, 8, num_relations=5, num_bases=%s, aggr=mean)" % num_bases


def test_layer_constructor_errors(wm_lib):
    from wholegraph_amd.torch.cugraphops import RGCNConv
    with pytest.raises(ValueError, match="Aggregation function"):
        RGCNConv(4, 4, 2, aggr="median")
    with pytest.raises(NotImplementedError):
        RGCNConv(4, 4, 2, aggr="max")
    with pytest.raises(ValueError, match="num_relations"):
        RGCNConv(4, 4, 0)
    with pytest.raises(ValueError, match="num_bases"):
        RGCNConv(4, 4, 2, num_bases=0)


def test_python_side_errors(wm_lib):
    import torch
    from wholegraph_amd.torch.cugraphops import RGCNConv
    from wholegraph_amd.torch.rel_aggregation import agg_concat_rel
    x = torch.zeros(5, 4)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    et = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(ValueError, match="aggr"):
        agg_concat_rel(x, rp, ci, et, 2, "median")
    with pytest.raises(NotImplementedError):
        agg_concat_rel(x, rp, ci, et, 2, "max")
    with pytest.raises(ValueError, match="num_relations"):
        agg_concat_rel(x, rp, ci, et, 0)
    with pytest.raises(TypeError, match="num_relations"):
        agg_concat_rel(x, rp, ci, et, 2.0)
    with pytest.raises(TypeError, match="float32"):
        agg_concat_rel(x.half(), rp, ci, et, 2)       # (no autocast region: a 16-bit x is refused)
    with pytest.raises(TypeError, match="float32"):
        agg_concat_rel(x.bfloat16(), rp, ci, et, 2)
    with pytest.raises(TypeError, match="float32"):
        agg_concat_rel(x.double(), rp, ci, et, 2)
    with pytest.raises(ValueError, match="2-D"):
        agg_concat_rel(x.reshape(-1), rp, ci, et, 2)
    with pytest.raises(TypeError, match="csr_row_ptr must be int32 or int64"):
        agg_concat_rel(x, rp.float(), ci, et, 2)
    with pytest.raises(ValueError, match="csr_col_ind must be 1-D"):
        agg_concat_rel(x, rp, ci.reshape(1, -1), et, 2)
    with pytest.raises(TypeError, match="edge_type must be int32 or int64"):
        agg_concat_rel(x, rp, ci, et.float(), 2)
    with pytest.raises(ValueError, match="edge_type must be 1-D"):
        agg_concat_rel(x, rp, ci, et.reshape(1, -1), 2)
    with pytest.raises(ValueError, match="edge_type is on"):
        agg_concat_rel(x, rp, ci, et.to("meta"), 2)
    with pytest.raises(ValueError, match="edge_type has 3 entries, csr_col_ind 0"):
        agg_concat_rel(x, rp, ci, torch.zeros(3, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="n_dst"):
        agg_concat_rel(x, torch.zeros(0, dtype=torch.int32), ci, et, 2)
    with pytest.raises(ValueError, match="more targets"):
        agg_concat_rel(x, torch.zeros(7, dtype=torch.int32), ci, et, 2)
    with pytest.raises(ValueError, match="at least one column"):
        agg_concat_rel(torch.zeros(5, 0), rp, ci, et, 2)
    with pytest.raises(ValueError, match="GPU"):
        agg_concat_rel(x, rp, ci, et, 2)       # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        RGCNConv(4, 3, 2)(x, rp, ci, 4, et)


def test_int64_types_that_int32_cannot_hold_stay_out_of_range(wm_lib):
    """an int64 type is narrowed to the op's int32: one that would wrap round into [0, R) must not become a valid type"""
    import torch
    from wholegraph_amd.torch.rel_aggregation import _edge_types
    t = torch.tensor([0, 2, 3, -1, 2 ** 32, 2 ** 32 + 1, -2 ** 32 + 1, 2 ** 40], dtype=torch.int64)
    got = _edge_types(t, 3, t.device)
    assert got.dtype == torch.int32 and got.tolist() == [0, 2, -1, -1, -1, -1, -1, -1]
    t32 = torch.tensor([0, 5, -7], dtype=torch.int32)
    assert _edge_types(t32, 3, t32.device).tolist() == [0, 5, -7]   # (int32 goes to the kernel as it is)


def test_model_name_rgcn(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import RGCNConv
    from wholegraph_amd.torch.gnn_model import create_rgcn_layers
    wgth.set_framework("cugraph")
    with pytest.raises(ValueError, match="create_rgcn_layers"):
        wgth.create_gnn_layers(32, 64, 5, 2, 1, "rgcn")
    layers = create_rgcn_layers(32, 64, 5, 3, 4)
    assert len(layers) == 3 and all(type(l) is RGCNConv for l in layers)
    assert [(l.in_channels, l.out_channels) for l in layers] == [(32, 64), (64, 64), (64, 5)]
    assert all(l.num_relations == 4 and l.num_bases is None and l.aggr == "mean" for l in layers)
    assert [l.num_bases for l in create_rgcn_layers(32, 64, 5, 2, 4, num_bases=2)] == [2, 2]
    emb = types.SimpleNamespace(shape=(100, 32))

    def args(**over):
        a = dict(hiddensize=64, layernum=2, model="rgcn", classnum=5, dropout=0.1, neighbors="5,5", num_relations=3,
                 edge_type_name="etype")
        a.update(over)
        return types.SimpleNamespace(**{k: v for k, v in a.items() if v is not None})

    with pytest.raises(ValueError, match="fuse_gather"):
        wgth.HomoGNNModel(None, emb, args(fuse_gather=True))
    with pytest.raises(ValueError, match="num_relations"):
        wgth.HomoGNNModel(None, emb, args(num_relations=None))
    with pytest.raises(ValueError, match="edge_type_name"):
        wgth.HomoGNNModel(None, emb, args(edge_type_name=None))


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
R, F, nd, ns = 2, 4, 2, 3
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
et = (C.c_int32 * 2)(1, 0)
x = (C.c_float * (ns * F))()
out = (C.c_float * (nd * (R + 1) * F))()
scale = (C.c_float * 2)()
gx = (C.c_float * (ns * F))()
env = L.wholememory_get_default_env_func()
W = (R + 1) * F
res = []
for aggr in (wmb.AGGR_SUM, wmb.AGGR_MEAN):
    res.append(L.wholememory_ext_csc_rel_aggregate_forward(row_ptr, col, et, 2, nd, ns, R, x, F, F, aggr, out, W, scale, env, None))
    res.append(L.wholememory_ext_csc_rel_aggregate_backward(row_ptr, col, et, 2, nd, ns, R, scale, out, W, F, aggr, gx, F, env,
                                                            None))
bad = [L.wholememory_ext_csc_rel_aggregate_forward(row_ptr, col, None, 2, nd, ns, R, x, F, F, wmb.AGGR_SUM, out, W, scale, env, None),
       L.wholememory_ext_csc_rel_aggregate_forward(row_ptr, col, et, 2, nd, ns, 0, x, F, F, wmb.AGGR_SUM, out, W, scale, env, None),
       L.wholememory_ext_csc_rel_aggregate_backward(row_ptr, col, et, 2, nd, ns, R, None, out, W, F, wmb.AGGR_MEAN, gx, F, env,
                                                    None),
       L.wholememory_ext_csc_rel_aggregate_backward(row_ptr, col, et, 2, nd, ns, R, scale, out, W - 1, F, wmb.AGGR_SUM, gx, F,
                                                    env, None)]
print("RESULT", *res, *bad)
'''


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    vals = [int(v) for v in line.split()[1:]]
    from wholegraph_amd import binding
    assert vals[:4] == [binding.NOT_SUPPORTED] * 4
    assert vals[4:] == [INV] * 4   # (the argument checks come first: a malformed call is INVALID_INPUT under every backend)


def test_entry_points_validate_arguments(wm_lib):
    """argument checks that come before any device work (the installed backend here is the product's: the calls are
    rejected before they could touch memory)"""
    import ctypes as C
    from wholegraph_amd import binding
    L = wm_lib
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(0, 1)
    et = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 256)()
    env = L.wholememory_get_default_env_func()
    R, F = 2, 4
    W = (R + 1) * F
    ok = dict(row_ptr=rp, col=col, et=et, E=2, nd=2, ns=3, R=R, x=buf, xs=F, F=F, aggr=binding.AGGR_MEAN, out=buf, os=W,
              scale=buf, g=buf, gs=W, gx=buf, gxs=F, env=env)

    def fwd(**over):
        a = dict(ok, **over)
        return getattr(L, FWD)(a["row_ptr"], a["col"], a["et"], a["E"], a["nd"], a["ns"], a["R"], a["x"], a["xs"], a["F"],
                               a["aggr"], a["out"], a["os"], a["scale"], a["env"], None)

    def bwd(**over):
        a = dict(ok, **over)
        return getattr(L, BWD)(a["row_ptr"], a["col"], a["et"], a["E"], a["nd"], a["ns"], a["R"], a["scale"], a["g"],
                               a["gs"], a["F"], a["aggr"], a["gx"], a["gxs"], a["env"], None)

    for fn in (fwd, bwd):
        for bad in (dict(row_ptr=None), dict(col=None), dict(et=None), dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4),
                    dict(R=0), dict(R=-3), dict(F=0), dict(aggr=2), dict(aggr=-1), dict(env=None), dict(scale=None),
                    dict(R=2 ** 31 - 1)):
            assert fn(**bad) == INV, bad
    assert fwd(x=None) == INV
    assert fwd(out=None) == INV
    assert fwd(xs=F - 1) == INV
    assert fwd(os=W - 1) == INV                # a row of out holds R + 1 slots of F columns
    assert bwd(g=None) == INV
    assert bwd(gx=None) == INV
    assert bwd(gs=W - 1) == INV
    assert bwd(gxs=F - 1) == INV
