"""The edge dot-product surface without a GPU: edge_dot_n2n, skipgram_block and Node2Vec importable from both package names;
the two C entry points exported, bound and stated in the header as section (2p); what is refused before any device work —
by the Python op (a row tensor that is not fp32, csr_row_ptr with no entry, x_dst with fewer rows than targets, no column)
and, under the CPU test backend, by the library (INVALID_INPUT for null pointers, a stride below F, F = 0, negative sizes);
and NOT_SUPPORTED for a well-formed call under that backend, whose entries for the op are null."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 6   # WHOLEMEMORY_INVALID_INPUT
NAMES = ("wholememory_ext_csc_edge_dot_forward", "wholememory_ext_csc_edge_dot_backward")


def test_names_importable_from_both_packages(wm_lib):
    import torch
    import pylibwholegraph.torch as pwt
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import edge_dot, node2vec, skipgram
    for pkg in (wgth, pwt):
        assert pkg.edge_dot_n2n is edge_dot.edge_dot_n2n
        assert pkg.skipgram_block is skipgram.skipgram_block and pkg.centers_of is skipgram.centers_of
        assert pkg.Node2Vec is node2vec.Node2Vec
    for name in ("edge_dot_n2n", "skipgram_block", "centers_of", "Node2Vec", "edge_dot", "skipgram", "node2vec"):
        assert name in wgth.__all__
    assert issubclass(edge_dot.CscEdgeDot, torch.autograd.Function) and issubclass(node2vec.Node2Vec, torch.nn.Module)
    E = inspect.Parameter.empty
    assert list(inspect.signature(edge_dot.edge_dot_n2n).parameters) == ["x_src", "x_dst", "csr_row_ptr", "csr_col_ind"]
    assert [(p.name, p.default) for p in inspect.signature(skipgram.skipgram_block).parameters.values()] == [
        ("walks", E), ("window", E), ("negatives", None)]
    params = list(inspect.signature(node2vec.Node2Vec.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [
        ("graph_structure", E), ("embedding", E), ("walk_length", E), ("window", E), ("num_negatives", E), ("p", 1.0),
        ("q", 1.0), ("weight_name", None), ("negative_mode", "uniform"), ("col_sorted", False), ("context_embedding", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[2:])
    for method in ("sample", "loss", "forward", "embed"):
        assert callable(getattr(node2vec.Node2Vec, method))


def test_symbols_exported_bound_and_stated_in_the_header(wm_lib):
    from wholegraph_amd import binding
    fwd, bwd = (binding.PROTOTYPES[n] for n in NAMES)
    assert len(fwd[1]) == 13 and len(bwd[1]) == 17
    assert all(hasattr(wm_lib, n) for n in NAMES)
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2p)") == 1
    o2, p2, seam = text.index("---- (2o)"), text.index("---- (2p)"), text.index("---- (3) testing seam")
    assert o2 < p2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2p)") == 1 and head.index("(2o)") < head.index("(2p)") < head.index("(3) the testing seam")
    for name in NAMES:
        assert text.count(name + "(") == 1 and p2 < text.index(name + "(") < seam


def test_python_side_errors(wm_lib, monkeypatch):
    """the checks in front of the op; those behind `is_cuda` are reached with CPU tensors by letting that one test pass"""
    import torch
    from wholegraph_amd.torch import edge_dot as ed
    F = 8
    x = torch.zeros(5, F)
    rp = torch.zeros(3, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        for args in ((x.to(dt), x), (x, x.to(dt))):
            with pytest.raises(TypeError, match="float32"):
                ed.edge_dot_n2n(*args, rp, ci)
    for args in ((x.reshape(-1), x), (x, x.reshape(-1))):
        with pytest.raises(ValueError, match="2-D"):
            ed.edge_dot_n2n(*args, rp, ci)
    with pytest.raises(ValueError, match="GPU"):
        ed.edge_dot_n2n(x, x, rp, ci)

    class Rows(torch.Tensor):
        is_cuda = True

    def rows(*shape):
        return torch.zeros(*shape).as_subclass(Rows)

    monkeypatch.setattr(ed.CscEdgeDot, "apply", staticmethod(lambda *a: pytest.fail("reached the op")))
    h = rows(5, F)
    with pytest.raises(ValueError, match="at least one column"):       # F = 0
        ed.edge_dot_n2n(rows(5, 0), rows(5, 0), rp, ci)
    with pytest.raises(ValueError, match="x_dst"):
        ed.edge_dot_n2n(h, rows(5, F + 1), rp, ci)
    with pytest.raises(ValueError, match="n_dst \\+ 1 >= 1"):          # row_ptr with no entry
        ed.edge_dot_n2n(h, h, torch.zeros(0, dtype=torch.int32), ci)
    with pytest.raises(ValueError, match="rows of x_dst"):             # fewer rows than targets
        ed.edge_dot_n2n(h, rows(1, F), rp, ci)
    with pytest.raises(TypeError, match="int32 or int64"):
        ed.edge_dot_n2n(h, h, rp.float(), ci)
    with pytest.raises(ValueError, match="1-D"):
        ed.edge_dot_n2n(h, h, rp, ci.reshape(1, -1))
    # more targets than source rows is the op's normal case, not an error
    monkeypatch.setattr(ed.CscEdgeDot, "apply", staticmethod(lambda *a: "reached"))
    assert ed.edge_dot_n2n(rows(1, F), h, rp, ci) == "reached"


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
F, nd, ns = 4, 3, 2                     # more targets than source rows
rp = (C.c_int32 * 4)(0, 1, 2, 3)
col = (C.c_int32 * 3)(1, 0, 1)
xs = (C.c_float * (ns * F))()
xd = (C.c_float * (nd * F))()
sc = (C.c_float * 3)()
gs = (C.c_float * (ns * F))()
gd = (C.c_float * (nd * F))()
env = L.wholememory_get_default_env_func()
ok = dict(rp=rp, col=col, E=3, nd=nd, ns=ns, xs=xs, xss=F, xd=xd, xds=F, F=F, sc=sc, g=sc, gs=gs, gss=F, gd=gd, gds=F, env=env)
def fwd(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csc_edge_dot_forward(a["rp"], a["col"], a["E"], a["nd"], a["ns"], a["xs"], a["xss"], a["xd"],
                                                  a["xds"], a["F"], a["sc"], a["env"], None)
def bwd(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csc_edge_dot_backward(a["rp"], a["col"], a["E"], a["nd"], a["ns"], a["xs"], a["xss"], a["xd"],
                                                   a["xds"], a["F"], a["g"], a["gs"], a["gss"], a["gd"], a["gds"], a["env"],
                                                   None)
both = [dict(rp=None), dict(col=None), dict(xs=None), dict(xd=None), dict(E=-1), dict(nd=-1), dict(ns=-1), dict(F=0),
        dict(F=-3), dict(F=2 ** 29), dict(xss=F - 1), dict(xds=F - 1), dict(env=None), dict(E=2 ** 31), dict(nd=2 ** 31)]
bad = [fn(**b) for fn in (fwd, bwd) for b in both]
bad += [fwd(sc=None), bwd(g=None), bwd(gs=None, gd=None), bwd(gss=F - 1), bwd(gds=F - 1)]
good = [fwd(), bwd(), bwd(gs=None), bwd(gd=None, gds=0), bwd(gs=None, gss=0), fwd(E=0, col=None, sc=None),
        fwd(nd=0, xd=None, col=None, sc=None), bwd(E=0, col=None, g=None), fwd(F=2 ** 29 - 1, xss=2 ** 29, xds=2 ** 29)]
print("RESULT", len(bad), *bad, *good)
'''


def test_argument_checks_come_first_then_not_supported_under_the_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    n_bad, *codes = (int(v) for v in line.split()[1:])
    bad, good = codes[:n_bad], codes[n_bad:]
    from wholegraph_amd import binding
    assert n_bad == 35 and bad == [INV] * n_bad, bad   # a malformed call is INVALID_INPUT under every backend
    assert len(good) == 9 and good == [binding.NOT_SUPPORTED] * 9, good   # the test backend's entries are null
