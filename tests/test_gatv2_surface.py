"""The GATv2 surface without a GPU: the two C entry points (exported, bound, stated in the header between (2f) and the
testing seam), NOT_SUPPORTED under the CPU test backend (which has no such kernels) and the argument checks that come
before any device work; names, signatures and parameter shapes of mha_gat_v2_n2n and GATv2Conv, the Python-side errors,
and the model name "gatv2" next to the still refused "gat"."""
import inspect
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 6   # WHOLEMEMORY_INVALID_INPUT


def test_symbols_exported_and_bound(wm_lib):
    from wholegraph_amd import binding
    fwd = binding.PROTOTYPES["wholememory_ext_csc_gatv2_forward"]
    bwd = binding.PROTOTYPES["wholememory_ext_csc_gatv2_backward"]
    assert len(fwd[1]) == 19 and len(bwd[1]) == 24
    assert hasattr(wm_lib, "wholememory_ext_csc_gatv2_forward") and hasattr(wm_lib, "wholememory_ext_csc_gatv2_backward")


def test_header_states_the_op_between_2f_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    f2, g2, seam = text.index("---- (2f)"), text.index("---- (2g)"), text.index("---- (3) testing seam")
    assert f2 < g2 < seam
    head = text[:text.index("#ifndef")]
    assert "(2g)" in head and head.index("(2g)") < head.index("(3) the testing seam")
    for name in ("wholememory_ext_csc_gatv2_forward", "wholememory_ext_csc_gatv2_backward"):
        assert g2 < text.index(name + "(") < seam


def test_exported_names_and_signatures(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gatv2_aggregation
    from wholegraph_amd.torch.cugraphops.gatv2_conv import GATv2Conv
    assert wgth.cugraphops.GATv2Conv is GATv2Conv and "GATv2Conv" in wgth.cugraphops.__all__
    assert "gatv2_aggregation" in wgth.__all__ and wgth.gatv2_aggregation is gatv2_aggregation
    assert issubclass(gatv2_aggregation.CscGatV2Conv, torch.autograd.Function)
    import pylibwholegraph.torch as pwt
    assert pwt.cugraphops.GATv2Conv is GATv2Conv and pwt.gatv2_aggregation is gatv2_aggregation
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(gatv2_aggregation.mha_gat_v2_n2n).parameters.values()] == [
        ("h_src", E), ("h_dst", E), ("att", E), ("csr_row_ptr", E), ("csr_col_ind", E), ("heads", E),
        ("negative_slope", 0.2), ("concat", True), ("return_alpha", False)]
    assert [(p.name, p.default) for p in list(inspect.signature(GATv2Conv.__init__).parameters.values())[1:]] == [
        ("in_channels", E), ("out_channels", E), ("heads", 1), ("concat", True), ("negative_slope", 0.2), ("bias", True),
        ("share_weights", False)]
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv
    assert list(inspect.signature(GATv2Conv.forward).parameters) == list(
        inspect.signature(CuGraphGATConv.forward).parameters)
    assert "edge_dim" in GATv2Conv.__doc__ and "not built" in GATv2Conv.__doc__


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_parameter_shapes(wm_lib, share, concat, bias):
    from wholegraph_amd.torch.cugraphops import GATv2Conv
    layer = GATv2Conv(16, 8, heads=3, concat=concat, bias=bias, share_weights=share)
    assert tuple(layer.lin_src.weight.shape) == (24, 16) and layer.lin_src.bias is None
    assert tuple(layer.lin_dst.weight.shape) == (24, 16) and layer.lin_dst.bias is None
    assert (layer.lin_dst is layer.lin_src) == share
    assert tuple(layer.att.shape) == (24,) and layer.att.abs().sum() > 0
    if bias:
        assert tuple(layer.bias.shape) == ((24,) if concat else (8,)) and not layer.bias.any()
    else:
        assert layer.bias is None
    names = sorted(n for n, _ in layer.named_parameters())
    want = ["lin_src.weight", "att"] + ([] if share else ["lin_dst.weight"]) + (["bias"] if bias else [])
    assert names == sorted(want)
    layer.reset_parameters()
    assert layer.heads == 3 and layer.concat == concat and layer.negative_slope == 0.2 and layer.share_weights == share
    assert repr(layer) == "GATv2Conv(16, 8, heads=3, share_weights=%s)" % share


def test_python_side_errors(wm_lib):
    import torch
    from wholegraph_amd.torch.cugraphops import GATv2Conv
    from wholegraph_amd.torch.gatv2_aggregation import mha_gat_v2_n2n
    H, F = 2, 4
    h = torch.zeros(5, H * F)
    att = torch.zeros(H * F)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(ValueError, match="heads"):
        mha_gat_v2_n2n(h, h, att, rp, ci, 0)
    with pytest.raises(TypeError, match="float32"):
        mha_gat_v2_n2n(h.half(), h, att, rp, ci, H)
    with pytest.raises(TypeError, match="float32"):
        mha_gat_v2_n2n(h, h.bfloat16(), att, rp, ci, H)
    with pytest.raises(TypeError, match="float32"):
        mha_gat_v2_n2n(h.double(), h, att, rp, ci, H)
    with pytest.raises(ValueError, match="2-D"):
        mha_gat_v2_n2n(h.reshape(-1), h, att, rp, ci, H)
    with pytest.raises(ValueError, match="GPU"):
        mha_gat_v2_n2n(h, h, att, rp, ci, H)       # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        GATv2Conv(3, F, heads=H)(torch.zeros(5, 3), rp, ci, 4)


def test_python_side_shape_errors_on_meta_free_checks(wm_lib, monkeypatch):
    """the checks behind `is_cuda`, reached with CPU tensors by letting that one test pass"""
    import torch
    from wholegraph_amd.torch import gatv2_aggregation as ga
    H, F = 2, 4

    class Rows(torch.Tensor):
        is_cuda = True

    def rows(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Rows)

    h = rows(5, H * F)
    att = torch.zeros(H * F)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    monkeypatch.setattr(ga.CscGatV2Conv, "apply", staticmethod(lambda *a: pytest.fail("reached the op")))
    with pytest.raises(ValueError, match="multiple of heads"):
        ga.mha_gat_v2_n2n(rows(5, 7), rows(5, 7), att, rp, ci, H)
    with pytest.raises(ValueError, match="h_dst"):
        ga.mha_gat_v2_n2n(h, rows(5, H * F + 1), att, rp, ci, H)
    with pytest.raises(ValueError, match="att"):
        ga.mha_gat_v2_n2n(h, h, torch.zeros(2 * H * F), rp, ci, H)
    with pytest.raises(ValueError, match="att"):
        ga.mha_gat_v2_n2n(h, h, att.double(), rp, ci, H)
    with pytest.raises(TypeError, match="int32 or int64"):
        ga.mha_gat_v2_n2n(h, h, att, rp.float(), ci, H)
    with pytest.raises(ValueError, match="1-D"):
        ga.mha_gat_v2_n2n(h, h, att, rp.reshape(1, -1), ci, H)
    with pytest.raises(ValueError, match="rows of h_src"):
        ga.mha_gat_v2_n2n(h, h, att, torch.zeros(7, dtype=torch.int32), ci, H)
    with pytest.raises(ValueError, match="rows of h_dst"):
        ga.mha_gat_v2_n2n(h, rows(1, H * F), att, rp, ci, H)


def test_model_name_gatv2_and_gat_still_refused(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import GATv2Conv
    wgth.set_framework("cugraph")
    layers = wgth.create_gnn_layers(32, 64, 5, 2, 4, "gatv2")
    assert len(layers) == 2 and all(type(l) is GATv2Conv for l in layers)
    assert [l.heads for l in layers] == [4, 4] and [l.concat for l in layers] == [True, False]
    assert (layers[0].in_channels, layers[0].out_channels) == (32, 16)
    assert (layers[1].in_channels, layers[1].out_channels) == (64, 5)
    with pytest.raises(NotImplementedError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gat")
    with pytest.raises(ValueError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gcn")
    args = types.SimpleNamespace(hiddensize=64, layernum=2, model="gatv2", classnum=5, dropout=0.1, neighbors="5,5",
                                 heads=4, fuse_gather=True)
    emb = types.SimpleNamespace(shape=(100, 32))
    with pytest.raises(ValueError, match="fuse_gather"):
        wgth.HomoGNNModel(None, emb, args)


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
H, F, nd, ns = 2, 4, 2, 3
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
h = (C.c_float * (ns * H * F))()
att = (C.c_float * (H * F))()
out = (C.c_float * (nd * H * F))()
alpha = (C.c_float * (2 * H))()
gs = (C.c_float * (ns * H * F))()
gd = (C.c_float * (nd * H * F))()
ga = (C.c_float * (H * F))()
env = L.wholememory_get_default_env_func()
fwd = L.wholememory_ext_csc_gatv2_forward(row_ptr, col, 2, nd, ns, h, H * F, h, H * F, att, H, F, 0.2, 1, out, H * F, alpha,
                                          env, None)
bwd = L.wholememory_ext_csc_gatv2_backward(row_ptr, col, 2, nd, ns, h, H * F, h, H * F, att, H, F, 0.2, 1, alpha, out,
                                           H * F, gs, H * F, gd, H * F, ga, env, None)
bad = [L.wholememory_ext_csc_gatv2_forward(row_ptr, col, 2, nd, ns, h, H * F, None, H * F, att, H, F, 0.2, 1, out, H * F,
                                           alpha, env, None),
       L.wholememory_ext_csc_gatv2_forward(row_ptr, col, 2, nd, ns, h, H * F, h, H * F, att, 0, F, 0.2, 1, out, H * F,
                                           alpha, env, None),
       L.wholememory_ext_csc_gatv2_backward(row_ptr, col, 2, nd, ns, h, H * F, None, H * F, att, H, F, 0.2, 1, alpha, out,
                                            H * F, gs, H * F, gd, H * F, ga, env, None),
       L.wholememory_ext_csc_gatv2_backward(row_ptr, col, 2, nd, ns, h, H * F, h, H * F, att, H, F, 0.2, 1, alpha, out,
                                            H * F, None, H * F, None, H * F, None, env, None)]
print("RESULT", fwd, bwd, *bad)
'''


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    fwd, bwd, *bad = (int(v) for v in line.split()[1:])
    from wholegraph_amd import binding
    assert fwd == binding.NOT_SUPPORTED and bwd == binding.NOT_SUPPORTED
    assert bad == [INV] * 4   # (the argument checks come first: a malformed call is INVALID_INPUT under every backend)


def test_entry_points_validate_arguments(wm_lib):
    """argument checks that come before any device work (the installed backend here is the product's: the calls are
    rejected before they could touch memory)"""
    import ctypes as C
    L = wm_lib
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 256)()
    env = L.wholememory_get_default_env_func()
    H, F = 2, 4
    ok = dict(row_ptr=rp, col=col, E=2, nd=2, ns=3, hs=buf, hss=H * F, hd=buf, hds=H * F, att=buf, H=H, F=F, concat=1,
              alpha=buf, out=buf, os=H * F, g=buf, gs=H * F, ghs=buf, ghss=H * F, ghd=buf, ghds=H * F, ga=buf, env=env)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gatv2_forward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["hs"], a["hss"],
                                                   a["hd"], a["hds"], a["att"], a["H"], a["F"], 0.2, a["concat"], a["out"],
                                                   a["os"], a["alpha"], a["env"], None)

    def bwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gatv2_backward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["hs"], a["hss"],
                                                    a["hd"], a["hds"], a["att"], a["H"], a["F"], 0.2, a["concat"],
                                                    a["alpha"], a["g"], a["gs"], a["ghs"], a["ghss"], a["ghd"], a["ghds"],
                                                    a["ga"], a["env"], None)

    for fn in (fwd, bwd):
        for bad in (dict(row_ptr=None), dict(col=None), dict(hs=None), dict(hd=None), dict(att=None), dict(alpha=None),
                    dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4), dict(H=0), dict(F=0), dict(hss=H * F - 1),
                    dict(hds=H * F - 1), dict(env=None)):
            assert fn(**bad) == INV, bad
    assert fwd(out=None) == INV
    assert fwd(os=H * F - 1) == INV
    assert fwd(concat=0, os=F - 1) == INV       # the mean over heads has rows of F floats
    assert bwd(g=None) == INV
    assert bwd(gs=H * F - 1) == INV
    assert bwd(concat=0, gs=F - 1) == INV
    assert bwd(ghs=None, ghd=None, ga=None) == INV   # no gradient asked for
    assert bwd(ghss=H * F - 1) == INV
    assert bwd(ghds=H * F - 1) == INV
