"""The edge-feature GAT surface without a GPU: names, signatures and defaults of mha_gat_n2n_edge and EdgeGATConv, parameter
shapes, the argument errors on CPU tensors, the unchanged signatures of mha_gat_n2n / CuGraphGATConv, and the two C entry
points: exported, bound, NOT_SUPPORTED under the CPU test backend (which has no such kernels) and their argument checks."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty


def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import edge_gat_aggregation
    from wholegraph_amd.torch.cugraphops.edge_gat_conv import EdgeGATConv
    assert wgth.cugraphops.EdgeGATConv is EdgeGATConv and "EdgeGATConv" in wgth.cugraphops.__all__
    assert "edge_gat_aggregation" in wgth.__all__ and wgth.edge_gat_aggregation is edge_gat_aggregation
    assert callable(edge_gat_aggregation.mha_gat_n2n_edge)
    assert issubclass(edge_gat_aggregation.CscGatEdgeConv, __import__("torch").autograd.Function)


def test_signatures(wm_lib):
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv, EdgeGATConv
    from wholegraph_amd.torch.edge_gat_aggregation import mha_gat_n2n_edge
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    assert [(p.name, p.default) for p in inspect.signature(mha_gat_n2n_edge).parameters.values()] == [
        ("h", EMPTY), ("att", EMPTY), ("edge_feat", EMPTY), ("csr_row_ptr", EMPTY), ("csr_col_ind", EMPTY),
        ("heads", EMPTY), ("negative_slope", 0.2), ("concat", True), ("return_alpha", False)]
    assert [(p.name, p.default) for p in list(inspect.signature(EdgeGATConv.__init__).parameters.values())[1:]] == [
        ("in_channels", EMPTY), ("out_channels", EMPTY), ("edge_dim", EMPTY), ("heads", 1), ("concat", True),
        ("negative_slope", 0.2), ("bias", True)]
    assert [(p.name, p.default) for p in inspect.signature(EdgeGATConv.forward).parameters.values()] == [
        ("self", EMPTY), ("x", EMPTY), ("csr_row_ptr", EMPTY), ("csr_col_ind", EMPTY), ("edge_attr", EMPTY),
        ("max_num_neighbors", None)]
    # the plain op and layer keep theirs
    assert [(p.name, p.default) for p in inspect.signature(mha_gat_n2n).parameters.values()] == [
        ("h", EMPTY), ("att", EMPTY), ("csr_row_ptr", EMPTY), ("csr_col_ind", EMPTY), ("heads", EMPTY),
        ("negative_slope", 0.2), ("concat", True), ("return_alpha", False)]
    assert [(p.name, p.default) for p in list(inspect.signature(CuGraphGATConv.__init__).parameters.values())[1:]] == [
        ("in_channels", EMPTY), ("out_channels", EMPTY), ("heads", 1), ("concat", True), ("negative_slope", 0.2),
        ("bias", True)]
    assert list(inspect.signature(CuGraphGATConv.forward).parameters) == ["self", "x", "csr_row_ptr", "csr_col_ind",
                                                                          "max_num_neighbors"]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_parameter_shapes(wm_lib, concat, bias):
    import torch
    from wholegraph_amd.torch.cugraphops import EdgeGATConv
    layer = EdgeGATConv(16, 8, 5, heads=3, concat=concat, bias=bias)
    assert tuple(layer.lin.weight.shape) == (24, 16) and layer.lin.bias is None
    assert tuple(layer.lin_edge.weight.shape) == (24, 5) and layer.lin_edge.bias is None
    assert tuple(layer.att.shape) == (72,)
    att = layer.att.detach().view(3, 3, 8)
    assert all(bool(att[half].any()) and bool(torch.isfinite(att[half]).all()) for half in range(3))
    if bias:
        assert tuple(layer.bias.shape) == ((24,) if concat else (8,)) and not layer.bias.any()
    else:
        assert layer.bias is None
    names = sorted(n for n, _ in layer.named_parameters())
    assert names == sorted(["lin.weight", "lin_edge.weight", "att"] + (["bias"] if bias else []))
    layer.reset_parameters()   # (no bias: nothing to zero)
    assert layer.heads == 3 and layer.concat == concat and layer.negative_slope == 0.2 and layer.edge_dim == 5
    assert repr(layer) == "EdgeGATConv(16, 8, edge_dim=5, heads=3)"


def test_argument_errors_on_cpu_tensors(wm_lib):
    import torch
    from wholegraph_amd.torch.cugraphops import EdgeGATConv
    from wholegraph_amd.torch.edge_gat_aggregation import mha_gat_n2n_edge
    H, F, E = 2, 4, 3
    h, att, ef = torch.zeros(5, H * F), torch.zeros(3 * H * F), torch.zeros(E, H * F)
    rp, ci = torch.tensor([0, 1, 3], dtype=torch.int32), torch.zeros(E, dtype=torch.int32)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32"):
            mha_gat_n2n_edge(h.to(dt), att, ef, rp, ci, H)
        with pytest.raises(TypeError, match="float32"):
            mha_gat_n2n_edge(h, att, ef.to(dt), rp, ci, H)
    with pytest.raises(ValueError, match="edge_feat"):
        mha_gat_n2n_edge(h, att, ef[:2], rp, ci, H)             # E - 1 rows
    with pytest.raises(ValueError, match="edge_feat"):
        mha_gat_n2n_edge(h, att, torch.zeros(E, H * F + 1), rp, ci, H)
    with pytest.raises(ValueError, match="att"):
        mha_gat_n2n_edge(h, att[:2 * H * F], ef, rp, ci, H)     # the plain op's att
    with pytest.raises(ValueError, match="heads"):
        mha_gat_n2n_edge(h, att, ef, rp, ci, 3)
    with pytest.raises(ValueError, match="heads"):
        mha_gat_n2n_edge(h, att, ef, rp, ci, 0)
    with pytest.raises(ValueError, match="GPU"):                # well-formed, but there is no CPU fallback
        mha_gat_n2n_edge(h, att, ef, rp, ci, H)
    layer = EdgeGATConv(5, F, 2, heads=H)
    with pytest.raises(ValueError, match="edge_attr"):
        layer(torch.zeros(5, 5), rp, ci, torch.zeros(E, 3))
    with pytest.raises(ValueError, match="edge_attr"):
        layer(torch.zeros(5, 5), rp, ci, torch.zeros(E))        # 1-D is [E, 1]: edge_dim is 2


def test_gat_models_still_refused(wm_lib):
    import wholegraph_amd.torch as wgth
    wgth.set_framework("cugraph")
    with pytest.raises(NotImplementedError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gat")


def test_symbols_exported_and_bound(wm_lib):
    from wholegraph_amd import binding
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("wholememory_ext_csc_gat_edge_forward", "wholememory_ext_csc_gat_edge_backward"):
        assert name in exported
        assert len(getattr(wm_lib, name).argtypes) == {"forward": 21, "backward": 26}[name.rsplit("_", 1)[1]]
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    assert header.index("(2e)") < header.index("(2f)") < header.index("(3) testing seam")
    assert "wholememory_ext_csc_gat_edge_backward(" in header


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
H, F, nd, ns, E = 2, 4, 2, 3, 2
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
h = (C.c_float * (ns * H * F))()
att = (C.c_float * (3 * H * F))()
ef = (C.c_float * (E * H * F))()
out = (C.c_float * (nd * H * F))()
alpha = (C.c_float * (E * H))()
es = (C.c_float * (E * H))()
scores = (C.c_float * ((ns + nd) * H))()
gh = (C.c_float * (ns * H * F))()
ga = (C.c_float * (3 * H * F))()
gef = (C.c_float * (E * H * F))()
env = L.wholememory_get_default_env_func()
fwd = L.wholememory_ext_csc_gat_edge_forward(row_ptr, col, E, nd, ns, h, H * F, att, ef, H * F, H, F, 0.2, 1, out, H * F,
                                             alpha, scores, es, env, None)
bwd = L.wholememory_ext_csc_gat_edge_backward(row_ptr, col, E, nd, ns, h, H * F, att, ef, H * F, H, F, 0.2, 1, alpha, scores,
                                              es, out, H * F, gh, H * F, ga, gef, H * F, env, None)
print("RESULT", fwd, bwd)
# a malformed call is judged before the backend is asked: a null row_ptr, a grad_edge_feat stride one short of the row
bad_fwd = L.wholememory_ext_csc_gat_edge_forward(None, col, E, nd, ns, h, H * F, att, ef, H * F, H, F, 0.2, 1, out, H * F,
                                                 alpha, scores, es, env, None)
bad_bwd = L.wholememory_ext_csc_gat_edge_backward(row_ptr, col, E, nd, ns, h, H * F, att, ef, H * F, H, F, 0.2, 1, alpha,
                                                  scores, es, out, H * F, gh, H * F, ga, gef, H * F - 1, env, None)
print("MALFORMED", bad_fwd, bad_bwd)
'''


def test_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    fwd, bwd = (int(v) for v in line.split()[1:])
    from wholegraph_amd import binding
    assert fwd == binding.NOT_SUPPORTED and bwd == binding.NOT_SUPPORTED
    malformed = [l for l in p.stdout.splitlines() if l.startswith("MALFORMED")][-1]
    assert [int(v) for v in malformed.split()[1:]] == [6, 6]   # WHOLEMEMORY_INVALID_INPUT


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
    ok = dict(row_ptr=rp, col=col, E=2, nd=2, ns=3, h=buf, hs=H * F, att=buf, ef=buf, efs=H * F, H=H, F=F, concat=1,
              alpha=buf, scores=buf, es=buf, out=buf, os=H * F, g=buf, gs=H * F, gh=buf, ghs=H * F, ga=buf, gef=buf,
              gefs=H * F)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gat_edge_forward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["h"], a["hs"],
                                                      a["att"], a["ef"], a["efs"], a["H"], a["F"], 0.2, a["concat"],
                                                      a["out"], a["os"], a["alpha"], a["scores"], a["es"], env, None)

    def bwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gat_edge_backward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["h"], a["hs"],
                                                       a["att"], a["ef"], a["efs"], a["H"], a["F"], 0.2, a["concat"],
                                                       a["alpha"], a["scores"], a["es"], a["g"], a["gs"], a["gh"],
                                                       a["ghs"], a["ga"], a["gef"], a["gefs"], env, None)

    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    for fn in (fwd, bwd):
        for bad in (dict(row_ptr=None), dict(col=None), dict(h=None), dict(att=None), dict(alpha=None),
                    dict(scores=None), dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4), dict(H=0), dict(F=0),
                    dict(hs=H * F - 1), dict(ef=None), dict(es=None), dict(efs=H * F - 1)):
            assert fn(**bad) == inv, bad
    assert fwd(out=None) == inv
    assert fwd(os=H * F - 1) == inv
    assert fwd(concat=0, os=F - 1) == inv       # the mean over heads has rows of F floats
    assert bwd(g=None) == inv
    assert bwd(gs=H * F - 1) == inv
    assert bwd(concat=0, gs=F - 1) == inv
    assert bwd(gh=None) == inv
    assert bwd(ghs=H * F - 1) == inv
    assert bwd(ga=None) == inv
    assert bwd(gef=None) == inv
    assert bwd(gefs=H * F - 1) == inv
