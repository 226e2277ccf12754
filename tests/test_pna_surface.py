"""The multi-aggregator surface without a GPU: the two C entry points (exported, bound, stated in the header between (2k)
and the testing seam), NOT_SUPPORTED under the CPU test backend (which has no such kernels) and the argument checks that
come before any device work; names, signatures and parameter shapes of agg_concat_pna and PNAConv, the Python-side errors,
create_pna_layers and the model name "pna"."""
import inspect
import math
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 6   # WHOLEMEMORY_INVALID_INPUT
NAMES = ("wholememory_ext_csc_pna_aggregate_forward", "wholememory_ext_csc_pna_aggregate_backward")


def test_symbols_exported_and_bound(wm_lib):
    from wholegraph_amd import binding
    fwd, bwd = (binding.PROTOTYPES[n] for n in NAMES)
    assert len(fwd[1]) == 18 and len(bwd[1]) == 19
    assert all(hasattr(wm_lib, n) for n in NAMES)
    assert binding.PNA_AGGR == {"sum": 1, "mean": 2, "min": 4, "max": 8, "std": 16}
    assert list(binding.PNA_AGGR) == ["sum", "mean", "min", "max", "std"]   # (the slot order)


def test_header_states_the_op_between_2k_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2l)") == 1
    k2, l2, seam = text.index("---- (2k)"), text.index("---- (2l)"), text.index("---- (3) testing seam")
    assert k2 < l2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2l)") == 1 and head.index("(2k)") < head.index("(2l)") < head.index("(3) the testing seam")
    for name in NAMES:
        assert text.count(name + "(") == 1 and l2 < text.index(name + "(") < seam
    section = " ".join(text[l2:seam].replace("\n *", "\n").split())   # (the comment's line breaks and their stars aside)
    for words in ("in the order SUM, MEAN, MIN, MAX, STD", "Only a strict comparison replaces", "the lowest edge position wins",
                  "a NaN in t_0 stays", "v = Q * r - m * m", "sqrtf((v > 0 ? v : 0) + eps)",
                  "A target without edges gets +0.0 in every aggregator slot, arg = -1",
                  "(G_std[d,f] * c[d,f]) * (x[s,f] - m[d,f])", "it is not added as a zero", "No per-target pre-pass",
                  "wholememory_ext_csc_aggregate_chunk_edges()", "NOT_SUPPORTED"):
        assert words in section, words
    for bit, value in (("SUM", 1), ("MEAN", 2), ("MIN", 4), ("MAX", 8), ("STD", 16)):
        assert "WHOLEMEMORY_EXT_PNA_%s = %d," % (bit, value) in section


def test_exported_names_and_signatures(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import pna_aggregation
    from wholegraph_amd.torch.cugraphops.pna_conv import PNAConv, pna_delta
    assert wgth.cugraphops.PNAConv is PNAConv and "PNAConv" in wgth.cugraphops.__all__
    assert wgth.cugraphops.pna_delta is pna_delta and "pna_delta" in wgth.cugraphops.__all__
    assert "pna_aggregation" in wgth.__all__ and wgth.pna_aggregation is pna_aggregation
    assert wgth.agg_concat_pna is pna_aggregation.agg_concat_pna
    assert wgth.create_pna_layers is wgth.gnn_model.create_pna_layers
    assert issubclass(pna_aggregation.CscAggregatePNA, torch.autograd.Function)
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(pna_aggregation.agg_concat_pna).parameters.values()] == [
        ("x", E), ("csr_row_ptr", E), ("csr_col_ind", E), ("aggregators", ("mean", "min", "max", "std")), ("eps", 1e-5)]
    assert [(p.name, p.default) for p in list(inspect.signature(PNAConv.__init__).parameters.values())[1:]] == [
        ("in_channels", E), ("out_channels", E), ("aggregators", ("mean", "min", "max", "std")),
        ("scalers", ("identity", "amplification", "attenuation")), ("delta", None), ("project", False),
        ("root_weight", True), ("bias", True)]
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    assert list(inspect.signature(PNAConv.forward).parameters) == list(inspect.signature(CuGraphSAGEConv.forward).parameters)
    assert [p for p in inspect.signature(wgth.create_pna_layers).parameters] == [
        "in_feat_dim", "hidden_feat_dim", "class_count", "num_layer", "delta", "aggregators", "scalers"]
    for words in ("one tower", "no per-edge pre-MLP", "edge_dim"):
        assert words in " ".join(PNAConv.__doc__.split()), words


def test_aggregator_lists(wm_lib):
    from wholegraph_amd.torch.pna_aggregation import aggregator_mask, aggregator_names
    assert aggregator_mask(["std", "sum", "max", "min", "mean"]) == 31
    assert aggregator_mask(("max",)) == 8 and aggregator_mask("max") == 8
    assert aggregator_names(aggregator_mask(["std", "min"])) == ["min", "std"]   # (slot order, not the caller's)
    for bad in ([], (), ["var"], ["mean", "median"], ["max", "max"], ["sum", "mean", "sum"], [None]):
        with pytest.raises(ValueError):
            aggregator_mask(bad)


def test_python_side_errors(wm_lib):
    import torch
    from wholegraph_amd.torch.cugraphops import PNAConv
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    x = torch.zeros(5, 4)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    for bad in ([], ["var"], ["max", "max"]):
        with pytest.raises(ValueError, match="aggregator"):
            agg_concat_pna(x, rp, ci, bad)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            agg_concat_pna(x.to(dt), rp, ci)
    with pytest.raises(ValueError, match="2-D"):
        agg_concat_pna(x.reshape(-1), rp, ci)
    with pytest.raises(ValueError, match="GPU"):
        agg_concat_pna(x, rp, ci)       # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        PNAConv(4, 3, scalers=["identity"])(x, rp, ci, 4)


def test_python_side_shape_errors_on_meta_free_checks(wm_lib, monkeypatch):
    """the checks behind `is_cuda`, reached with CPU tensors by letting that one test pass"""
    import torch
    from wholegraph_amd.torch import pna_aggregation as pa

    class Rows(torch.Tensor):
        is_cuda = True

    x = torch.zeros(5, 4).as_subclass(Rows)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    monkeypatch.setattr(pa.CscAggregatePNA, "apply", staticmethod(lambda *a: pytest.fail("reached the op")))
    with pytest.raises(TypeError, match="int32 or int64"):
        pa.agg_concat_pna(x, rp.float(), ci)
    with pytest.raises(TypeError, match="int32 or int64"):
        pa.agg_concat_pna(x, rp, ci.float())
    with pytest.raises(ValueError, match="1-D"):
        pa.agg_concat_pna(x, rp.reshape(1, -1), ci)
    with pytest.raises(ValueError, match="1-D"):
        pa.agg_concat_pna(x, rp, ci.reshape(1, -1))
    with pytest.raises(ValueError, match="more targets"):
        pa.agg_concat_pna(x, torch.zeros(7, dtype=torch.int32), ci)
    with pytest.raises(ValueError, match="at least one column"):
        pa.agg_concat_pna(torch.zeros(5, 0).as_subclass(Rows), rp, ci)
    with pytest.raises(ValueError, match="eps"):
        pa.agg_concat_pna(x, rp, ci, eps=-1.0)


def test_layer_argument_errors(wm_lib):
    from wholegraph_amd.torch.cugraphops import PNAConv
    for bad in ([], ["var"], ["min", "min"]):
        with pytest.raises(ValueError, match="aggregator"):
            PNAConv(8, 4, aggregators=bad, delta=1.0)
    for bad in ([], ["linear"], ["identity", "identity"]):
        with pytest.raises(ValueError, match="scaler"):
            PNAConv(8, 4, scalers=bad, delta=1.0)
    for scalers in (["amplification"], ["identity", "attenuation"], ("identity", "amplification", "attenuation")):
        with pytest.raises(ValueError, match="delta"):
            PNAConv(8, 4, scalers=scalers)
    for delta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="delta"):
            PNAConv(8, 4, delta=delta)
    assert PNAConv(8, 4, scalers=["identity"]).delta is None   # (identity alone needs none)
    layer = PNAConv(8, 4, aggregators=["std", "max"], scalers="amplification", delta=2)
    assert layer.aggregators == ["max", "std"] and layer.scalers == ["amplification"] and layer.delta == 2.0


@pytest.mark.parametrize("project", [True, False])
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("aggregators,scalers", [(("mean", "min", "max", "std"), ("identity", "amplification", "attenuation")),
                                                 (("max",), ("identity",)),
                                                 (("sum", "mean", "min", "max", "std"), ("identity", "attenuation"))])
def test_parameter_shapes(wm_lib, project, root, bias, aggregators, scalers):
    from wholegraph_amd.torch.cugraphops import PNAConv
    layer = PNAConv(16, 8, aggregators=aggregators, scalers=scalers, delta=1.5, project=project, root_weight=root, bias=bias)
    want = {"lin.weight": (8, (len(aggregators) * len(scalers) + (1 if root else 0)) * 16)}
    if bias:
        want["lin.bias"] = (8,)
    if project:
        want["pre_lin.weight"], want["pre_lin.bias"] = (16, 16), (16,)
    else:
        assert layer.pre_lin is None
    assert {n: tuple(p.shape) for n, p in layer.named_parameters()} == want
    layer.reset_parameters()
    assert (layer.in_channels, layer.out_channels, layer.root_weight) == (16, 8, root)
    assert repr(layer).startswith("PNAConv(16, 8, aggregators=[")


def test_pna_delta(wm_lib):
    import torch
    from wholegraph_amd.torch.cugraphops import pna_delta
    rp = torch.tensor([0, 0, 1, 4, 4, 11], dtype=torch.int32)
    want = sum(math.log(d + 1) for d in (0, 1, 3, 0, 7)) / 5
    assert abs(pna_delta(rp) - want) < 1e-12 and isinstance(pna_delta(rp), float)
    assert abs(pna_delta(rp.long()) - want) < 1e-12
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32)):
        with pytest.raises(ValueError):
            pna_delta(bad)


def test_model_surface(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import PNAConv
    wgth.set_framework("cugraph")
    layers = wgth.create_pna_layers(32, 64, 5, 3, 1.25)
    assert len(layers) == 3 and all(type(l) is PNAConv for l in layers)
    assert [(l.in_channels, l.out_channels) for l in layers] == [(32, 64), (64, 64), (64, 5)]
    assert all(l.aggregators == ["mean", "min", "max", "std"] and l.delta == 1.25 and l.root_weight for l in layers)
    assert all(l.scalers == ["identity", "amplification", "attenuation"] and l.pre_lin is None for l in layers)
    assert [tuple(l.lin.weight.shape) for l in layers] == [(64, 13 * 32), (64, 13 * 64), (5, 13 * 64)]
    layers = wgth.create_pna_layers(32, 64, 5, 2, None, aggregators=["max"], scalers=["identity"])
    assert [tuple(l.lin.weight.shape) for l in layers] == [(64, 2 * 32), (5, 2 * 64)]
    with pytest.raises(ValueError, match="delta"):
        wgth.create_pna_layers(32, 64, 5, 2, None)
    # create_gnn_layers has no place for delta: it keeps refusing the name, in its own words
    with pytest.raises(ValueError, match="'sage', 'gatv2' and 'transformer'"):
        wgth.create_gnn_layers(32, 64, 5, 2, 1, "pna")
    emb = types.SimpleNamespace(shape=(100, 32))
    base = dict(hiddensize=64, layernum=2, model="pna", classnum=5, dropout=0.1, neighbors="5,5")
    with pytest.raises(ValueError, match="pna_delta"):
        wgth.HomoGNNModel(None, emb, types.SimpleNamespace(**base))
    with pytest.raises(ValueError, match="fuse_gather"):
        wgth.HomoGNNModel(None, emb, types.SimpleNamespace(pna_delta=1.0, fuse_gather=True, **base))
    with pytest.raises(ValueError, match="aggregator"):
        wgth.HomoGNNModel(None, emb, types.SimpleNamespace(pna_delta=1.0, pna_aggregators=["var"], **base))
    with pytest.raises(ValueError, match="scaler"):
        wgth.HomoGNNModel(None, emb, types.SimpleNamespace(pna_delta=1.0, pna_scalers=["linear"], **base))


def test_existing_ops_keep_refusing_max_and_min(wm_lib):
    from wholegraph_amd.torch.aggregation import aggr_code
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError):
            aggr_code(aggr)
        with pytest.raises(NotImplementedError):
            CuGraphSAGEConv(8, 4, aggr=aggr)


_CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
os.environ["WHOLEGRAPH_AMD_TESTING"] = "1"
from wholegraph_amd import binding as wmb
L = wmb.lib()
if sys.argv[2] == "oracle":
    tb = C.CDLL(os.path.join(sys.argv[1], "oracle", "libwm_test_backend.so"))
    tb.wm_test_backend.restype = C.c_void_p
    wmb.check(L.wm_testing_install_backend(C.c_void_p(tb.wm_test_backend())))
    assert L.wholememory_ext_backend_name().startswith(b"oracle-test-backend")
else:
    assert L.wholememory_ext_backend_name() == b"hip-gfx950"
F, nd, ns, E = 4, 2, 3, 2
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
x = (C.c_float * (ns * F))()
out = (C.c_float * (nd * 6 * F))()
ai = (C.c_int32 * (nd * F))()
sf = (C.c_float * (nd * F))()
gx = (C.c_float * (ns * F))()
env = L.wholememory_get_default_env_func()
ok = dict(rp=row_ptr, col=col, E=E, nd=nd, ns=ns, x=x, xs=F, F=F, mask=31, eps=1e-5, out=out, os=6 * F, amin=ai, amax=ai, m=sf,
          c=sf, g=out, gs=6 * F, gx=gx, gxs=F, env=env)
def fwd(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csc_pna_aggregate_forward(a["rp"], a["col"], a["E"], a["nd"], a["ns"], a["x"], a["xs"], a["F"],
                                                       a["mask"], a["eps"], a["out"], a["os"], a["amin"], a["amax"], a["m"],
                                                       a["c"], a["env"], None)
def bwd(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csc_pna_aggregate_backward(a["rp"], a["col"], a["E"], a["nd"], a["ns"], a["x"], a["xs"], a["F"],
                                                        a["mask"], a["amin"], a["amax"], a["m"], a["c"], a["g"], a["gs"],
                                                        a["gx"], a["gxs"], a["env"], None)
both = [dict(rp=None), dict(col=None), dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4), dict(F=0), dict(mask=0),
        dict(mask=32), dict(mask=-1), dict(mask=8, os=2 * F - 1, gs=2 * F - 1), dict(os=6 * F - 1, gs=6 * F - 1),
        dict(xs=F - 1, gxs=F - 1)]
bad = [fn(**b) for fn in (fwd, bwd) for b in both]
bad += [fwd(x=None), fwd(out=None), fwd(eps=-1.0), fwd(eps=float("nan"))]
bad += [bwd(g=None), bwd(gx=None), bwd(env=None), bwd(x=None), bwd(mask=16, x=None, gs=2 * F), bwd(amin=None),
        bwd(amax=None), bwd(m=None), bwd(c=None), bwd(mask=16, xs=F - 1)]
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [fwd(), bwd(), fwd(mask=8, amin=None, amax=None, m=None, c=None), bwd(mask=3, x=None, amin=None, amax=None, m=None,
                                                                                   c=None)]
print("RESULT", len(bad), *bad, *good)
'''


def _child(backend):
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, backend], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    n, *codes = (int(v) for v in line.split()[1:])
    return codes[:n], codes[n:]


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    bad, good = _child("oracle")
    from wholegraph_amd import binding
    assert len(bad) == 40 and bad == [INV] * len(bad)   # (the argument checks come first, whatever the backend)
    assert good == [binding.NOT_SUPPORTED] * 4


def test_entry_points_validate_arguments_under_the_product_backend(wm_lib):
    """the same malformed calls with the product's backend installed: rejected before they could touch memory"""
    bad, good = _child("hip")
    assert len(bad) == 40 and bad == [INV] * len(bad) and good == []
