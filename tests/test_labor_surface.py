"""The LABOR sampler's surface without a GPU: the prototype, the argument checks of the C entry point (header section 2v) on
wrapped host tensors under the product backend and the CPU test backend (NOT_SUPPORTED to a well-formed call), and the
Python-side argument errors."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_prototype(wm_lib):
    from wholegraph_amd import binding
    vp, i = C.c_void_p, C.c_int
    assert binding.PROTOTYPES["wholememory_ext_csr_labor_sample"] == (
        i, [vp, vp, vp, i, i, C.c_ulonglong, vp, vp, vp, vp, C.POINTER(binding.EnvFunc), vp])


_CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from wholegraph_amd import binding as wmb
L = wmb.lib()
if sys.argv[2] == "oracle":
    tb = C.CDLL(os.path.join(sys.argv[1], "oracle", "libwm_test_backend.so"))
    tb.wm_test_backend.restype = C.c_void_p
    wmb.check(L.wm_testing_install_backend(C.c_void_p(tb.wm_test_backend())))
DT = {np.dtype(np.int32): wmb.DT_INT, np.dtype(np.int64): wmb.DT_INT64, np.dtype(np.float32): wmb.DT_FLOAT}
keep = []
def wrap(a, shape=None):      # a host array as a wholememory tensor (never read here); shape: what the description claims
    keep.append(np.ascontiguousarray(a))
    desc = wmb.make_tensor_desc(list(a.shape if shape is None else shape), DT[a.dtype])
    h = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(h), C.c_void_p(keep[-1].ctypes.data), C.byref(desc)))
    return h
n_nodes, n_edges, n, i64, i32, f32 = 5, 7, 4, np.int64, np.int32, np.float32
env, ctx = wmb.EnvFunc(), C.c_void_p(1)      # (never called / opaque: every answer comes before the first allocation)
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), nodes=wrap(np.zeros(n, i64)), M=5, mode=0,
          off=wrap(np.zeros(n + 1, i32)), dctx=ctx, opt=None, env=C.byref(env))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_labor_sample(a["row"], a["col"], a["nodes"], a["M"], a["mode"], 77, a["off"], a["dctx"], a["opt"],
                                              a["opt"], a["env"], None)
many = (1 << 31) - 1      # (a description over a one-entry array: refused before anything is read)
row32, colf, off64 = wrap(np.zeros(n_nodes + 1, i32)), wrap(np.zeros(n_edges, f32)), wrap(np.zeros(n + 1, i64))
invalid = [call(row=None), call(col=None), call(nodes=None), call(off=None), call(dctx=None), call(env=None),
           call(row=wrap(np.zeros((2, 3), i64))), call(nodes=wrap(np.zeros((2, 2), i64))), call(off=wrap(np.zeros((n + 1, 1), i32))),
           call(M=65), call(M=0, mode=1), call(M=-1, mode=1), call(mode=2), call(mode=-1), call(row=wrap(np.zeros(0, i64))),
           call(nodes=wrap(np.zeros(1, i64), [many]), off=wrap(np.zeros(1, i32), [many + 1])), call(off=wrap(np.zeros(n, i32))),
           # and two faults, one of shape, size or scalar and one of dtype: the former's answer
           call(M=65, row=row32), call(mode=2, col=colf), call(off=wrap(np.zeros(n, i64))), call(dctx=None, col=colf)]
logic = [call(row=row32), call(col=colf), call(nodes=wrap(np.zeros(n, f32))), call(off=off64), call(row=row32, off=off64)]
good = []      # (under the product backend a well-formed call would reach the device)
if sys.argv[2] == "oracle":
    good = [call(), call(opt=ctx), call(nodes=wrap(np.zeros(n, i32))), call(M=64), call(M=-1), call(M=1, mode=1),
            call(M=(1 << 31) - 1, mode=1), call(nodes=wrap(np.zeros(0, i64)))]
print("RESULT", len(invalid), len(logic), *invalid, *logic, *good)
'''


@pytest.mark.parametrize("backend", ["oracle", "hip"])
def test_argument_checks_in_the_stated_order(wm_lib, backend):
    """the same malformed calls under both backends: answered before any device work (the product's has no device here)"""
    from wholegraph_amd import binding
    if backend == "oracle":
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, backend], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    a, b, *codes = (int(v) for v in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:])
    assert (a, b) == (21, 5) and codes[:a] == [INV] * a and codes[a:a + b] == [LOGIC] * b
    assert codes[a + b:] == ([binding.NOT_SUPPORTED] * 8 if backend == "oracle" else [])


@pytest.mark.parametrize("kwargs", [dict(mode="uniform"), dict(max_sample_count=65), dict(max_sample_count=0, mode="poisson"),
                                    dict(max_sample_count=1 << 31, mode="poisson"), dict(dim=2)], ids=str)
def test_python_side_argument_errors(wm_lib, kwargs):
    import torch
    from wholegraph_amd.torch import wholegraph_ops
    a = dict(dict(max_sample_count=5, mode="fixed", dim=1), **kwargs)
    with pytest.raises(ValueError):      # (before the graph tensors are looked at)
        wholegraph_ops.labor_sample(None, None, torch.zeros((3,) * a["dim"], dtype=torch.int64), a["max_sample_count"], 1, a["mode"])
