"""topk_rows' surface without a GPU: the prototype, the argument checks of the C entry point (header section 2x) on wrapped
host tensors under the product backend and the CPU test backend (NOT_SUPPORTED to a well-formed call), and the Python-side
argument errors. The malformed calls are those that differ from section 2w, and one per error class of the shared ones."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_prototype(wm_lib):
    from wholegraph_amd import binding
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert binding.PROTOTYPES["wholememory_ext_topk_rows"] == (
        i, [vp, vp, i, i, i64, i64, vp, vp, vp, vp, C.POINTER(binding.EnvFunc), vp])


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
DT = {np.dtype(np.int32): wmb.DT_INT, np.dtype(np.int64): wmb.DT_INT64, np.dtype(np.float32): wmb.DT_FLOAT,
      np.dtype(np.float64): wmb.DT_DOUBLE}
keep = []
def wrap(a, shape=None, strides=None):      # a host array as a wholememory tensor (never read here); shape: what the description claims
    keep.append(np.ascontiguousarray(a))
    desc = wmb.make_tensor_desc(list(a.shape if shape is None else shape), DT[a.dtype], strides, 0)
    h = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(h), C.c_void_p(keep[-1].ctypes.data), C.byref(desc)))
    return h
N, F, B, M, K, i64, i32, f32 = 9, 5, 4, 6, 3, np.int64, np.int32, np.float32
env = wmb.EnvFunc()      # (never called: every answer comes before the first allocation)
ok = dict(table=wrap(np.zeros((N, F), f32)), query=wrap(np.zeros((B, F), f32)), k=K, measure=0, begin=0, end=N, frow=None,
          fids=None, ids=wrap(np.zeros((B, K), i64)), scores=wrap(np.zeros((B, K), f32)), env=C.byref(env))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_topk_rows(a["table"], a["query"], a["k"], a["measure"], a["begin"], a["end"], a["frow"], a["fids"],
                                       a["ids"], a["scores"], a["env"], None)
frow, fids, tablef64 = wrap(np.zeros(B + 1, i64)), wrap(np.zeros(M, i64)), wrap(np.zeros((N, F), np.float64))
big = wrap(np.zeros((1, 1), f32), [(1 << 31) + 1, 1])      # (a description over a small array: refused before anything is read)
invalid = [call(table=None), call(ids=None), call(scores=None), call(env=None), call(frow=frow), call(ids=wrap(np.zeros(B * K, i64))),
           call(scores=wrap(np.zeros(B, f32))), call(k=0), call(k=65), call(k=-1), call(ids=wrap(np.zeros((B, K + 1), i64))),
           call(ids=wrap(np.zeros((B + 1, K), i64))), call(scores=wrap(np.zeros((B - 1, K), f32))),
           call(ids=wrap(np.zeros((B, K), i64), None, [K - 1, 1])),
           call(table=big, query=wrap(np.zeros((B, 1), f32)), end=(1 << 31) + 1), call(end=N + 1), call(measure=3),
           call(frow=wrap(np.zeros(B, i64)), fids=fids),
           # and two faults, one of shape, size or scalar and one of dtype: the former's answer
           call(k=65, table=tablef64), call(ids=wrap(np.zeros((B, K + 1), i32))), call(measure=-1, scores=wrap(np.zeros((B, K), np.float64)))]
logic = [call(table=tablef64), call(ids=wrap(np.zeros((B, K), i32))), call(scores=wrap(np.zeros((B, K), np.float64))),
         call(frow=wrap(np.zeros(B + 1, f32)), fids=fids), call(frow=frow, fids=wrap(np.zeros(M, f32)))]
good = []      # (under the product backend a well-formed call would reach the device)
if sys.argv[2] == "oracle":
    good = [call(), call(k=1, ids=wrap(np.zeros((B, 1), i64)), scores=wrap(np.zeros((B, 1), f32))), call(measure=2, frow=frow, fids=fids),
            call(frow=wrap(np.zeros(B + 1, i32)), fids=wrap(np.zeros(M, i32))), call(frow=frow, fids=wrap(np.zeros(M, i32))),
            call(begin=2, end=2), call(ids=wrap(np.zeros((B, K + 2), i64), [B, K], [K + 2, 1])),
            call(query=wrap(np.zeros((0, F), f32)), ids=wrap(np.zeros((0, K), i64)), scores=wrap(np.zeros((0, K), f32)))]
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


@pytest.mark.parametrize("kwargs", [dict(measure="cosine"), dict(filter_row_ptr=0), dict(filter_ids=0), dict(k=0), dict(k=65)], ids=str)
def test_python_side_argument_errors(wm_lib, kwargs):
    import torch
    from wholegraph_amd.torch import wholegraph_ops
    with pytest.raises(ValueError):      # (before the table is looked at)
        wholegraph_ops.topk_rows(None, torch.zeros(3, 4), **dict(dict(k=5), **kwargs))
