"""The scaled dot-product attention surface without a GPU: the two C entry points (exported, bound, stated in the header
between (2j) and the testing seam), NOT_SUPPORTED under the CPU test backend (which has no such kernels) and the argument
checks that come before any device work; names, signatures and parameter shapes of mha_simple_n2n and TransformerConv, the
Python-side errors, and the model name "transformer" next to the still refused "gat"."""
import inspect
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 6   # WHOLEMEMORY_INVALID_INPUT
NAMES = ("wholememory_ext_csc_mha_simple_forward", "wholememory_ext_csc_mha_simple_backward")


def test_symbols_exported_and_bound(wm_lib):
    from wholegraph_amd import binding
    fwd, bwd = (binding.PROTOTYPES[n] for n in NAMES)
    assert len(fwd[1]) == 20 and len(bwd[1]) == 26
    assert all(hasattr(wm_lib, n) for n in NAMES)


def test_header_states_the_op_between_2j_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2k)") == 1
    j2, k2, seam = text.index("---- (2j)"), text.index("---- (2k)"), text.index("---- (3) testing seam")
    assert j2 < k2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2k)") == 1 and head.index("(2j)") < head.index("(2k)") < head.index("(3) the testing seam")
    for name in NAMES:
        assert text.count(name + "(") == 1 and k2 < text.index(name + "(") < seam


def test_exported_names_and_signatures(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import transformer_aggregation
    from wholegraph_amd.torch.cugraphops.transformer_conv import TransformerConv
    assert wgth.cugraphops.TransformerConv is TransformerConv and "TransformerConv" in wgth.cugraphops.__all__
    assert "transformer_aggregation" in wgth.__all__ and wgth.transformer_aggregation is transformer_aggregation
    assert issubclass(transformer_aggregation.CscMhaSimple, torch.autograd.Function)
    import pylibwholegraph.torch as pwt
    assert pwt.cugraphops.TransformerConv is TransformerConv and pwt.transformer_aggregation is transformer_aggregation
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(transformer_aggregation.mha_simple_n2n).parameters.values()] == [
        ("key_emb", E), ("query_emb", E), ("value_emb", E), ("csr_row_ptr", E), ("csr_col_ind", E), ("heads", E),
        ("concat", True), ("norm_by_dim", True), ("return_alpha", False)]
    assert [(p.name, p.default) for p in list(inspect.signature(TransformerConv.__init__).parameters.values())[1:]] == [
        ("in_channels", E), ("out_channels", E), ("heads", 1), ("concat", True), ("beta", False), ("bias", True),
        ("root_weight", True)]
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv
    assert list(inspect.signature(TransformerConv.forward).parameters) == list(
        inspect.signature(CuGraphGATConv.forward).parameters)
    assert "edge_dim" in TransformerConv.__doc__ and "dropout" in TransformerConv.__doc__
    assert "not built" in TransformerConv.__doc__


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("beta", [True, False])
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_parameter_shapes(wm_lib, concat, beta, root, bias):
    from wholegraph_amd.torch.cugraphops import TransformerConv
    if beta and not root:
        with pytest.raises(ValueError, match="root_weight"):
            TransformerConv(16, 8, heads=3, concat=concat, beta=beta, bias=bias, root_weight=root)
        return
    layer = TransformerConv(16, 8, heads=3, concat=concat, beta=beta, bias=bias, root_weight=root)
    width = 24 if concat else 8
    want = {}
    for name in ("lin_key", "lin_query", "lin_value"):   # (always with bias)
        want[name + ".weight"], want[name + ".bias"] = (24, 16), (24,)
    if root:
        want["lin_skip.weight"] = (width, 16)
        if bias:
            want["lin_skip.bias"] = (width,)
    else:
        assert layer.lin_skip is None
    if beta:
        want["lin_beta.weight"] = (1, 3 * width)
    else:
        assert layer.lin_beta is None
    assert {n: tuple(p.shape) for n, p in layer.named_parameters()} == want
    layer.reset_parameters()
    assert (layer.heads, layer.concat, layer.beta, layer.root_weight) == (3, concat, beta, root)
    assert (layer.in_channels, layer.out_channels) == (16, 8)
    assert repr(layer) == "TransformerConv(16, 8, heads=3)"


def test_python_side_errors(wm_lib):
    import torch
    from wholegraph_amd.torch.cugraphops import TransformerConv
    from wholegraph_amd.torch.transformer_aggregation import mha_simple_n2n
    H, F = 2, 4
    h = torch.zeros(5, H * F)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(ValueError, match="heads"):
        mha_simple_n2n(h, h, h, rp, ci, 0)
    for i in range(3):
        for dt in (torch.float16, torch.bfloat16, torch.float64):
            args = [h, h, h]
            args[i] = h.to(dt)
            with pytest.raises(TypeError, match="float32"):
                mha_simple_n2n(*args, rp, ci, H)
        args = [h, h, h]
        args[i] = h.reshape(-1)
        with pytest.raises(ValueError, match="2-D"):
            mha_simple_n2n(*args, rp, ci, H)
    with pytest.raises(ValueError, match="GPU"):
        mha_simple_n2n(h, h, h, rp, ci, H)       # CPU tensors
    with pytest.raises(ValueError, match="GPU"):
        TransformerConv(3, F, heads=H)(torch.zeros(5, 3), rp, ci, 4)


def test_python_side_shape_errors_on_meta_free_checks(wm_lib, monkeypatch):
    """the checks behind `is_cuda`, reached with CPU tensors by letting that one test pass"""
    import torch
    from wholegraph_amd.torch import transformer_aggregation as ta
    H, F = 2, 4

    class Rows(torch.Tensor):
        is_cuda = True

    def rows(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Rows)

    h = rows(5, H * F)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    monkeypatch.setattr(ta.CscMhaSimple, "apply", staticmethod(lambda *a: pytest.fail("reached the op")))
    with pytest.raises(ValueError, match="multiple of heads"):
        ta.mha_simple_n2n(rows(5, 7), rows(5, 7), rows(5, 7), rp, ci, H)
    with pytest.raises(ValueError, match="query_emb"):
        ta.mha_simple_n2n(h, rows(5, H * F + 1), h, rp, ci, H)
    with pytest.raises(ValueError, match="value_emb"):
        ta.mha_simple_n2n(h, h, rows(5, H * F + 1), rp, ci, H)
    with pytest.raises(ValueError, match="value_emb"):
        ta.mha_simple_n2n(h, h, rows(4, H * F), rp, ci, H)
    with pytest.raises(TypeError, match="int32 or int64"):
        ta.mha_simple_n2n(h, h, h, rp.float(), ci, H)
    with pytest.raises(TypeError, match="int32 or int64"):
        ta.mha_simple_n2n(h, h, h, rp, ci.float(), H)
    with pytest.raises(ValueError, match="1-D"):
        ta.mha_simple_n2n(h, h, h, rp.reshape(1, -1), ci, H)
    with pytest.raises(ValueError, match="rows of key_emb"):
        ta.mha_simple_n2n(h, h, h, torch.zeros(7, dtype=torch.int32), ci, H)
    with pytest.raises(ValueError, match="rows of query_emb"):
        ta.mha_simple_n2n(h, rows(1, H * F), h, rp, ci, H)


def test_model_name_transformer_and_gat_still_refused(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import TransformerConv
    wgth.set_framework("cugraph")
    layers = wgth.create_gnn_layers(32, 64, 5, 2, 4, "transformer")
    assert len(layers) == 2 and all(type(l) is TransformerConv for l in layers)
    assert [l.heads for l in layers] == [4, 4] and [l.concat for l in layers] == [True, False]
    assert (layers[0].in_channels, layers[0].out_channels) == (32, 16)
    assert (layers[1].in_channels, layers[1].out_channels) == (64, 5)
    assert all(l.root_weight and not l.beta for l in layers)
    with pytest.raises(NotImplementedError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gat")
    with pytest.raises(ValueError, match="'sage', 'gatv2' and 'transformer'"):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gcn")
    args = types.SimpleNamespace(hiddensize=64, layernum=2, model="transformer", classnum=5, dropout=0.1, neighbors="5,5",
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
HF = H * F
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
h = (C.c_float * (ns * HF))()
out = (C.c_float * (nd * HF))()
alpha = (C.c_float * (2 * H))()
gk = (C.c_float * (ns * HF))()
gq = (C.c_float * (nd * HF))()
gv = (C.c_float * (ns * HF))()
env = L.wholememory_get_default_env_func()
F_ = L.wholememory_ext_csc_mha_simple_forward
B_ = L.wholememory_ext_csc_mha_simple_backward
fwd = F_(row_ptr, col, 2, nd, ns, h, HF, h, HF, h, HF, H, F, 1, 1, out, HF, alpha, env, None)
bwd = B_(row_ptr, col, 2, nd, ns, h, HF, h, HF, h, HF, H, F, 1, 1, alpha, out, HF, gk, HF, gq, HF, gv, HF, env, None)
bad = [F_(row_ptr, col, 2, nd, ns, h, HF, None, HF, h, HF, H, F, 1, 1, out, HF, alpha, env, None),
       F_(row_ptr, col, 2, nd, ns, h, HF, h, HF, h, HF, 0, F, 1, 1, out, HF, alpha, env, None),
       B_(row_ptr, col, 2, nd, ns, h, HF, h, HF, None, HF, H, F, 1, 1, alpha, out, HF, gk, HF, gq, HF, gv, HF, env, None),
       B_(row_ptr, col, 2, nd, ns, h, HF, h, HF, h, HF, H, F, 1, 1, alpha, out, HF, None, HF, None, HF, None, HF, env, None)]
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
    HF = H * F
    ok = dict(row_ptr=rp, col=col, E=2, nd=2, ns=3, k=buf, ks=HF, q=buf, qs=HF, v=buf, vs=HF, H=H, F=F, norm=1, concat=1,
              alpha=buf, out=buf, os=HF, g=buf, gs=HF, gk=buf, gks=HF, gq=buf, gqs=HF, gv=buf, gvs=HF, env=env)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_mha_simple_forward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["k"], a["ks"],
                                                        a["q"], a["qs"], a["v"], a["vs"], a["H"], a["F"], a["norm"],
                                                        a["concat"], a["out"], a["os"], a["alpha"], a["env"], None)

    def bwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_mha_simple_backward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["k"], a["ks"],
                                                         a["q"], a["qs"], a["v"], a["vs"], a["H"], a["F"], a["norm"],
                                                         a["concat"], a["alpha"], a["g"], a["gs"], a["gk"], a["gks"],
                                                         a["gq"], a["gqs"], a["gv"], a["gvs"], a["env"], None)

    for fn in (fwd, bwd):
        for bad in (dict(row_ptr=None), dict(col=None), dict(k=None), dict(q=None), dict(v=None), dict(alpha=None),
                    dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4), dict(H=0), dict(F=0), dict(ks=HF - 1),
                    dict(qs=HF - 1), dict(vs=HF - 1), dict(env=None)):
            assert fn(**bad) == INV, bad
    assert fwd(out=None) == INV
    assert fwd(os=HF - 1) == INV
    assert fwd(concat=0, os=F - 1) == INV       # the mean over heads has rows of F floats
    assert bwd(g=None) == INV
    assert bwd(gs=HF - 1) == INV
    assert bwd(concat=0, gs=F - 1) == INV
    assert bwd(gk=None, gq=None, gv=None) == INV   # no gradient asked for
    assert bwd(gks=HF - 1) == INV
    assert bwd(gqs=HF - 1) == INV
    assert bwd(gvs=HF - 1) == INV
