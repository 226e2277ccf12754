"""The per-relation sampler's surface without a GPU: the argument checks of the C entry point (header section 2t) on wrapped
host tensors — shapes, sizes and scalars before dtypes, pinned by calls with two faults — under the product backend and the CPU
test backend (NOT_SUPPORTED to a well-formed call); csrc/tysample.hpp on the host (tests/cpp/tysample_test.cpp); the model."""
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_the_rules_of_the_header_on_the_host(tmp_path):
    exe = str(tmp_path / "tysample_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "tysample_test.cpp"), "-o", exe], capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    out = subprocess.run([exe], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-4000:])


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
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), ty=wrap(np.zeros(n_edges, i32)),
          nodes=wrap(np.zeros(n, i64)), f=[3, 0, 5], off=wrap(np.zeros(n + 1, i32)), dctx=ctx, opt=None, env=C.byref(env))
def call(**over):
    a = dict(ok, **over)
    f = None if a["f"] is None else (C.c_int * max(len(a["f"]), 1))(*a["f"])
    return L.wholememory_ext_csr_typed_sample(a["row"], a["col"], a["ty"], a["nodes"], a.get("R", len(a["f"] or [])), f, 77, a["off"],
                                              a["dctx"], a["opt"], a["opt"], a["opt"], a["env"], None)
many = (1 << 31) // 8      # n * F = 2^31 with F = 8 (a description over a one-entry array: refused before anything is read)
big = dict(nodes=wrap(np.zeros(1, i64), [many]), off=wrap(np.zeros(1, i32), [many + 1]))
row32, colf, ty64, off64 = wrap(np.zeros(n_nodes + 1, i32)), wrap(np.zeros(n_edges, f32)), wrap(np.zeros(n_edges, i64)), wrap(np.zeros(n + 1, i64))
invalid = [call(row=None), call(col=None), call(ty=None), call(nodes=None), call(off=None), call(f=None, R=3), call(dctx=None),
           call(env=None), call(row=wrap(np.zeros((2, 3), i64))), call(ty=wrap(np.zeros((7, 1), i32))),
           call(nodes=wrap(np.zeros((2, 2), i64))), call(off=wrap(np.zeros((n + 1, 1), i32))),
           call(R=0), call(f=[1] * 65), call(f=[-1, 2]), call(f=[65]), call(f=[0, 0]), call(f=[32, 32, 1]), call(**big),
           call(ty=wrap(np.zeros(n_edges - 1, i32))), call(ty=wrap(np.zeros(n_edges + 1, i32))), call(off=wrap(np.zeros(n, i32))),
           # and two faults, one of shape, size or scalar and one of dtype: the former's answer
           call(R=0, ty=ty64), call(f=[65], row=row32), call(ty=wrap(np.zeros(n_edges - 1, i64))), call(off=wrap(np.zeros(n, i64))), call(dctx=None, col=colf)]
logic = [call(row=row32), call(col=colf), call(nodes=wrap(np.zeros(n, f32))), call(ty=ty64), call(ty=wrap(np.zeros(n_edges, f32))),
         call(off=off64), call(row=row32, off=off64), call(ty=ty64, opt=ctx)]
good = []      # (under the product backend a well-formed call would reach the device)
if sys.argv[2] == "oracle":
    good = [call(), call(opt=ctx), call(nodes=wrap(np.zeros(n, i32))), call(f=[64]), call(f=[1] * 64),
            call(nodes=wrap(np.zeros(1, i64), [many - 1]), off=wrap(np.zeros(1, i32), [many])), call(nodes=wrap(np.zeros(0, i64)))]
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
    assert (a, b) == (27, 8) and codes[:a] == [INV] * a and codes[a:a + b] == [LOGIC] * b
    assert codes[a + b:] == ([binding.NOT_SUPPORTED] * 7 if backend == "oracle" else [])


def test_relation_fanouts_on_the_model(wm_lib):
    from wholegraph_amd.torch import gnn_model
    check = gnn_model._checked_relation_fanouts
    assert check(None, 2, 3) is None and check([(1, 2, 3), [0, 0, 4]], 2, 3) == [[1, 2, 3], [0, 0, 4]]
    for bad in ([[1, 2, 3]], [[1, 2], [1, 2]], [[1, 2, 3], [0, 0, 0]], [[1, 2, 3], [60, 5, 0]], [[1, 2, 3], [-1, 2, 3]]):
        with pytest.raises(ValueError):
            check(bad, 2, 3)
    args = types.SimpleNamespace(hiddensize=8, layernum=2, model="rgcn", classnum=3, dropout=0.0, neighbors="5,5", num_relations=3,
                                 edge_type_name="ty", relation_fanouts=[[1, 2, 3]])
    with pytest.raises(ValueError, match="relation_fanouts"):
        gnn_model.HomoGNNModel(None, types.SimpleNamespace(shape=(10, 4)), args)
