"""The fp16 / bf16 surface of the GraphSAGE aggregation without a GPU: the two `_typed` entry points and their bound
argument types, NOT_SUPPORTED under the CPU test backend (which has no such kernels), the argument checks that come before
any device work, and the dtype checks of `agg_concat`."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = ("wholememory_ext_csc_aggregate_forward_typed", "wholememory_ext_csc_aggregate_backward_typed")


def test_typed_symbols_exist_with_bound_argument_types(wm_lib):
    from wholegraph_amd import binding
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    want = [vp, vp, i64, i64, i64, vp, i64, i64, i, vp, i64, i, C.POINTER(binding.EnvFunc), vp]
    for name in TYPED:
        restype, argtypes = binding.PROTOTYPES[name]
        assert restype is i and list(argtypes) == want, name
        fn = getattr(wm_lib, name)
        assert fn.restype is i and list(fn.argtypes) == want, name
    # the untyped entry points keep their signatures: the typed ones are theirs plus the dtype
    for name in TYPED:
        _, plain = binding.PROTOTYPES[name.replace("_typed", "")]
        assert list(plain) == want[:11] + want[12:]
    assert (binding.DT_FLOAT, binding.DT_HALF, binding.DT_BF16) == (1, 2, 4)


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
F, nd, ns = 8, 2, 3
row_ptr = (C.c_int32 * 3)(0, 1, 2)
col = (C.c_int32 * 2)(2, 0)
x = (C.c_uint16 * (ns * F))()
out = (C.c_uint16 * (nd * 2 * F))()
gx = (C.c_uint16 * (ns * F))()
env = L.wholememory_get_default_env_func()
res = []
for dt in (wmb.DT_HALF, wmb.DT_BF16):
    res.append(L.wholememory_ext_csc_aggregate_forward_typed(row_ptr, col, 2, nd, ns, x, F, F, wmb.AGGR_MEAN, out, 2 * F, dt,
                                                             env, None))
    res.append(L.wholememory_ext_csc_aggregate_backward_typed(row_ptr, col, 2, nd, ns, out, 2 * F, F, wmb.AGGR_SUM, gx, F, dt,
                                                              env, None))
print("RESULT", *res)
# a malformed call is judged before the backend is asked: a null row_ptr, a grad_x stride one short of the row
bad_fwd = L.wholememory_ext_csc_aggregate_forward_typed(None, col, 2, nd, ns, x, F, F, wmb.AGGR_MEAN, out, 2 * F, wmb.DT_HALF,
                                                        env, None)
bad_bwd = L.wholememory_ext_csc_aggregate_backward_typed(row_ptr, col, 2, nd, ns, out, 2 * F, F, wmb.AGGR_SUM, gx, F - 1,
                                                         wmb.DT_BF16, env, None)
print("MALFORMED", bad_fwd, bad_bwd)
'''


def test_typed_entry_points_not_supported_under_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    from wholegraph_amd import binding
    assert [int(v) for v in line.split()[1:]] == [binding.NOT_SUPPORTED] * 4
    malformed = [l for l in p.stdout.splitlines() if l.startswith("MALFORMED")][-1]
    assert [int(v) for v in malformed.split()[1:]] == [6, 6]   # WHOLEMEMORY_INVALID_INPUT


def test_typed_entry_points_validate_arguments(wm_lib):
    """the checks of the fp32 entry points, for every row dtype, plus the dtype itself (the installed backend here is the
    product's: the calls are rejected before they could touch memory)"""
    from wholegraph_amd import binding
    L = wm_lib
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 64)()
    env = L.wholememory_get_default_env_func()
    ok = dict(row_ptr=rp, col=col, E=2, nd=2, ns=3, x=buf, xs=8, dim=8, aggr=binding.AGGR_MEAN, out=buf, os=16,
              dt=binding.DT_HALF)

    def call(fn, **over):
        a = dict(ok, **over)
        return fn(a["row_ptr"], a["col"], a["E"], a["nd"], a["ns"], a["x"], a["xs"], a["dim"], a["aggr"], a["out"], a["os"],
                  a["dt"], env, None)

    fwd, bwd = (getattr(L, n) for n in TYPED)
    inv = 6   # WHOLEMEMORY_INVALID_INPUT
    for fn in (fwd, bwd):
        for dt in (binding.DT_DOUBLE, binding.DT_INT, binding.DT_UNKNOWN, binding.DT_INT64, binding.DT_INT16,
                   binding.DT_INT8, binding.DT_COUNT):
            assert call(fn, dt=dt) == inv, dt
        for dt in (binding.DT_FLOAT, binding.DT_HALF, binding.DT_BF16):
            assert call(fn, dt=dt, row_ptr=None) == inv
            assert call(fn, dt=dt, col=None) == inv
            assert call(fn, dt=dt, x=None) == inv
            assert call(fn, dt=dt, out=None) == inv
            assert call(fn, dt=dt, E=-1) == inv
            assert call(fn, dt=dt, nd=-1) == inv
            assert call(fn, dt=dt, ns=-1) == inv
            assert call(fn, dt=dt, nd=4) == inv           # more targets than rows of x
            assert call(fn, dt=dt, dim=0) == inv
            assert call(fn, dt=dt, aggr=7) == inv
    for dt in (binding.DT_FLOAT, binding.DT_HALF, binding.DT_BF16):
        assert call(fwd, dt=dt, xs=7) == inv               # x rows of 8 elements
        assert call(fwd, dt=dt, os=15) == inv              # out rows of 16 elements
        assert call(bwd, dt=dt, xs=15) == inv              # grad_out rows of 16 elements
        assert call(bwd, dt=dt, os=7) == inv               # grad_x rows of 8 elements


def test_backward_typed_needs_env_functions(wm_lib):
    from wholegraph_amd import binding
    rp = (C.c_int32 * 3)(0, 1, 2)
    col = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 64)()
    for dt in (binding.DT_HALF, binding.DT_BF16):
        assert wm_lib.wholememory_ext_csc_aggregate_backward_typed(rp, col, 2, 2, 3, buf, 16, 8, binding.AGGR_SUM, buf, 8, dt,
                                                                   None, None) == 6


def test_agg_concat_dtype_checks_without_a_gpu(wm_lib):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    rp, ci = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([2, 0], dtype=torch.int32)
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        with pytest.raises(ValueError, match="GPU tensor"):
            agg_concat(torch.zeros((3, 8), dtype=dt), rp, ci)
    for dt in (torch.float64, torch.int32, torch.int8):
        with pytest.raises(TypeError):
            agg_concat(torch.zeros((3, 8), dtype=dt), rp, ci)
    # the GAT op stays fp32 only: 16-bit h is a TypeError outside autocast
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32"):
            mha_gat_n2n(torch.zeros((3, 8), dtype=dt), torch.zeros(16), rp, ci, 1)
