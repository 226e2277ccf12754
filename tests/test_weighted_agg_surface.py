"""The edge-weighted aggregation surface without a GPU: names and signatures, argument errors that come before any device
work, the two C entry points under the CPU test backend (which has no such kernels: NOT_SUPPORTED, no crash) and their
argument checks, and the two symbols in the ABI."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wholememory_ext_csc_aggregate_weighted_forward", "wholememory_ext_csc_aggregate_weighted_backward")


def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import weighted_aggregation
    from wholegraph_amd.torch.cugraphops.weighted_sage_conv import EdgeWeightedSAGEConv
    assert wgth.cugraphops.EdgeWeightedSAGEConv is EdgeWeightedSAGEConv
    assert wgth.cugraphops.__all__[-1] == "EdgeWeightedSAGEConv"
    assert wgth.cugraphops.__all__[:2] == ["CuGraphSAGEConv", "CuGraphGATConv"]
    assert "weighted_aggregation" in wgth.__all__ and wgth.weighted_aggregation is weighted_aggregation
    assert callable(weighted_aggregation.agg_concat_weighted)
    assert callable(wgth.GraphStructure.multilayer_sample_with_edge_attributes)


def test_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv, EdgeWeightedSAGEConv
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    assert [(p.name, p.default) for p in inspect.signature(agg_concat_weighted).parameters.values()] == [
        ("x", inspect.Parameter.empty), ("csr_row_ptr", inspect.Parameter.empty), ("csr_col_ind", inspect.Parameter.empty),
        ("edge_weight", inspect.Parameter.empty), ("aggr", "mean")]
    init = lambda cls: [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert init(EdgeWeightedSAGEConv) == init(CuGraphSAGEConv) == [
        ("in_channels", inspect.Parameter.empty), ("out_channels", inspect.Parameter.empty), ("aggr", "mean"),
        ("normalize", False), ("root_weight", True), ("project", False), ("bias", True)]
    assert list(inspect.signature(EdgeWeightedSAGEConv.forward).parameters) == [
        "self", "x", "csr_row_ptr", "csr_col_ind", "max_num_neighbors", "edge_weight"]
    ps = list(inspect.signature(wgth.GraphStructure.multilayer_sample_with_edge_attributes).parameters.values())
    assert [(p.name, p.kind) for p in ps][1:] == [
        ("node_ids", inspect.Parameter.POSITIONAL_OR_KEYWORD), ("max_neighbors", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("edge_attr_names", inspect.Parameter.POSITIONAL_OR_KEYWORD), ("weight_name", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("random_seeds", inspect.Parameter.KEYWORD_ONLY)]
    assert ps[4].default is None and ps[5].default is None


@pytest.mark.parametrize("root_weight,project,bias", [(True, False, True), (False, True, False)])
def test_layer_parameters_are_those_of_the_sage_layer(wm_lib, root_weight, project, bias):
    import torch
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv, EdgeWeightedSAGEConv
    torch.manual_seed(3)
    a = EdgeWeightedSAGEConv(16, 8, root_weight=root_weight, project=project, bias=bias)
    torch.manual_seed(3)
    b = CuGraphSAGEConv(16, 8, root_weight=root_weight, project=project, bias=bias)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert sorted(pa) == sorted(pb)
    for name in pa:
        assert torch.equal(pa[name], pb[name]), name      # same shapes, same initialisation from the same seed
    assert repr(a) == "EdgeWeightedSAGEConv(16, 8, aggr=mean)"
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError):
            EdgeWeightedSAGEConv(8, 4, aggr=aggr)
    with pytest.raises(ValueError):
        EdgeWeightedSAGEConv(8, 4, aggr="median")


def test_argument_errors_come_before_any_device_work(wm_lib):
    """host tensors throughout: every check below fires before the op would touch a device"""
    import torch
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    x = torch.zeros(4, 8)
    rp, ci = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([3, 0], dtype=torch.int32)
    w = torch.ones(2)
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError):
            agg_concat_weighted(x, rp, ci, w, aggr)
    with pytest.raises(ValueError):
        agg_concat_weighted(x, rp, ci, w, "median")
    for bad in (x.half(), x.bfloat16(), x.double()):
        with pytest.raises(TypeError, match="float32"):
            agg_concat_weighted(bad, rp, ci, w)
    with pytest.raises(ValueError):
        agg_concat_weighted(x[0], rp, ci, w)
    with pytest.raises(TypeError):
        agg_concat_weighted(x, rp.float(), ci, w)
    with pytest.raises(ValueError):
        agg_concat_weighted(x, rp.reshape(1, 3), ci, w)
    with pytest.raises(TypeError, match="edge_weight must be float32"):
        agg_concat_weighted(x, rp, ci, w.half())
    with pytest.raises(ValueError, match="edge_weight must be 1-D"):
        agg_concat_weighted(x, rp, ci, w.reshape(2, 1))
    with pytest.raises(ValueError, match="edge_weight has 3 entries"):
        agg_concat_weighted(x, rp, ci, torch.ones(3))
    with pytest.raises(ValueError, match="more targets"):
        agg_concat_weighted(x[:1], rp, ci, w)
    with pytest.raises(ValueError, match="GPU tensor"):
        agg_concat_weighted(x, rp, ci, w)


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
w = (C.c_float * 2)(1.0, 2.0)
x = (C.c_float * (ns * F))()
out = (C.c_float * (nd * 2 * F))()
gx = (C.c_float * (ns * F))()
gw = (C.c_float * 2)()
env = L.wholememory_get_default_env_func()
fwd = L.wholememory_ext_csc_aggregate_weighted_forward(row_ptr, col, w, 2, nd, ns, x, F, F, 1, out, 2 * F, env, None)
bwd = L.wholememory_ext_csc_aggregate_weighted_backward(row_ptr, col, 2, nd, ns, x, F, w, out, 2 * F, F, 1, gx, F, gw, env,
                                                        None)
print("RESULT", fwd, bwd)
# a malformed call is judged before the backend is asked: a null row_ptr, a grad_out stride one short of the row
bad_fwd = L.wholememory_ext_csc_aggregate_weighted_forward(None, col, w, 2, nd, ns, x, F, F, 1, out, 2 * F, env, None)
bad_bwd = L.wholememory_ext_csc_aggregate_weighted_backward(row_ptr, col, 2, nd, ns, x, F, w, out, 2 * F - 1, F, 1, gx, F, gw,
                                                            env, None)
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
    F = 4
    ok = dict(row_ptr=rp, col=col, w=buf, E=2, nd=2, ns=3, x=buf, xs=F, F=F, aggr=1, out=buf, os=2 * F, g=buf, gs=2 * F,
              gx=buf, gxs=F, gw=buf, env=env)

    def fwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_aggregate_weighted_forward(a["row_ptr"], a["col"], a["w"], a["E"], a["nd"], a["ns"],
                                                                a["x"], a["xs"], a["F"], a["aggr"], a["out"], a["os"],
                                                                a["env"], None)

    def bwd(**over):
        a = dict(ok, **over)
        return L.wholememory_ext_csc_aggregate_weighted_backward(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["x"],
                                                                 a["xs"], a["w"], a["g"], a["gs"], a["F"], a["aggr"],
                                                                 a["gx"], a["gxs"], a["gw"], a["env"], None)

    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    for fn in (fwd, bwd):
        for bad in (dict(row_ptr=None), dict(col=None), dict(w=None), dict(E=-1), dict(nd=-1), dict(ns=-1), dict(nd=4),
                    dict(F=0), dict(aggr=2), dict(aggr=-1), dict(x=None), dict(xs=F - 1)):
            assert fn(**bad) == inv, (fn.__name__, bad)
    assert fwd(out=None) == inv
    assert fwd(os=2 * F - 1) == inv
    assert bwd(g=None) == inv
    assert bwd(gs=2 * F - 1) == inv
    assert bwd(gxs=F - 1) == inv
    assert bwd(gx=None, gw=None) == inv           # one of the two gradients must be asked for
    assert bwd(env=None) == inv


def test_the_two_symbols_are_the_only_new_exports(wm_lib):
    """declared in the header, exported by the library, bound in binding.PROTOTYPES — and the library's export list holds
    nothing outside the headers (so nothing else came with them)"""
    import re
    from wholegraph_amd import binding
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header) and name in exported and name in binding.PROTOTYPES
        assert getattr(wm_lib, name) is not None
    weighted = sorted(n for n in exported if "weighted" in n and "aggregate" in n)
    assert weighted == sorted(NEW_SYMBOLS)
    assert "(2d)" in header
