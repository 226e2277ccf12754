"""The GAT layer surface without a GPU: names and signatures of the reference's CuGraphGATConv, parameter shapes, the
models that still refuse gat, and the GAT entry points under the CPU test backend (which has no such kernels:
NOT_SUPPORTED, no crash) and their argument checks."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gat_aggregation
    from wholegraph_amd.torch.cugraphops.gat_conv import CuGraphGATConv
    assert wgth.cugraphops.CuGraphGATConv is CuGraphGATConv
    assert "CuGraphGATConv" in wgth.cugraphops.__all__ and "gat_aggregation" in wgth.__all__
    assert wgth.gat_aggregation is gat_aggregation
    assert callable(gat_aggregation.mha_gat_n2n) and callable(gat_aggregation.node_chunk)


def test_signatures(wm_lib):
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    sig = inspect.signature(CuGraphGATConv.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty), ("heads", 1),
        ("concat", True), ("negative_slope", 0.2), ("bias", True)]
    assert list(inspect.signature(CuGraphGATConv.forward).parameters) == ["self", "x", "csr_row_ptr", "csr_col_ind",
                                                                          "max_num_neighbors"]
    assert [(p.name, p.default) for p in inspect.signature(mha_gat_n2n).parameters.values()][4:] == [
        ("heads", inspect.Parameter.empty), ("negative_slope", 0.2), ("concat", True), ("return_alpha", False)]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_parameter_shapes(wm_lib, concat, bias):
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv
    layer = CuGraphGATConv(16, 8, heads=3, concat=concat, bias=bias)
    assert tuple(layer.lin.weight.shape) == (24, 16) and layer.lin.bias is None
    assert tuple(layer.att.shape) == (48,)
    if bias:
        assert tuple(layer.bias.shape) == ((24,) if concat else (8,)) and not layer.bias.any()
    else:
        assert layer.bias is None
    names = sorted(n for n, _ in layer.named_parameters())
    assert names == sorted(["lin.weight", "att"] + (["bias"] if bias else []))
    layer.reset_parameters()   # (no bias: nothing to zero)
    assert layer.heads == 3 and layer.concat == concat and layer.negative_slope == 0.2
    assert repr(layer) == "CuGraphGATConv(16, 8, heads=3)"


def test_gat_models_still_refused(wm_lib):
    import wholegraph_amd.torch as wgth
    wgth.set_framework("cugraph")
    with pytest.raises(NotImplementedError):
        wgth.create_gnn_layers(32, 64, 5, 2, 4, "gat")


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
att = (C.c_float * (2 * H * F))()
out = (C.c_float * (nd * H * F))()
alpha = (C.c_float * (2 * H))()
scores = (C.c_float * ((ns + nd) * H))()
gh = (C.c_float * (ns * H * F))()
ga = (C.c_float * (2 * H * F))()
env = L.wholememory_get_default_env_func()
fwd = L.wholememory_ext_csc_gat_forward(row_ptr, col, 2, nd, ns, h, H * F, att, H, F, 0.2, 1, out, H * F, alpha, scores,
                                        env, None)
bwd = L.wholememory_ext_csc_gat_backward(row_ptr, col, 2, nd, ns, h, H * F, att, H, F, 0.2, 1, alpha, scores, out, H * F,
                                         gh, H * F, ga, env, None)
print("RESULT", fwd, bwd, L.wholememory_ext_csc_gat_node_chunk())
# a malformed call is judged before the backend is asked: a null row_ptr, a grad_h stride one short of the row
bad_fwd = L.wholememory_ext_csc_gat_forward(None, col, 2, nd, ns, h, H * F, att, H, F, 0.2, 1, out, H * F, alpha, scores, env,
                                            None)
bad_bwd = L.wholememory_ext_csc_gat_backward(row_ptr, col, 2, nd, ns, h, H * F, att, H, F, 0.2, 1, alpha, scores, out, H * F,
                                             gh, H * F - 1, ga, env, None)
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
    L = wm_lib
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 256)()
    env = L.wholememory_get_default_env_func()
    H, F = 2, 4
    ok = dict(row_ptr=rp, col=col, E=2, nd=2, ns=3, h=buf, hs=H * F, att=buf, H=H, F=F, concat=1, alpha=buf, scores=buf,
              out=buf, os=H * F, g=buf, gs=H * F, gh=buf, ghs=H * F, ga=buf)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gat_forward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["h"], a["hs"],
                                                 a["att"], a["H"], a["F"], 0.2, a["concat"], a["out"], a["os"],
                                                 a["alpha"], a["scores"], env, None)

    def bwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_gat_backward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["h"], a["hs"],
                                                  a["att"], a["H"], a["F"], 0.2, a["concat"], a["alpha"], a["scores"],
                                                  a["g"], a["gs"], a["gh"], a["ghs"], a["ga"], env, None)

    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    for fn in (fwd, bwd):
        for bad in (dict(row_ptr=None), dict(col=None), dict(h=None), dict(att=None), dict(alpha=None),
                    dict(scores=None), dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4), dict(H=0), dict(F=0),
                    dict(hs=H * F - 1)):
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
