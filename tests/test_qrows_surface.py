"""The surface of the 8-bit row-quantized tables (wholegraph_amd_ext.h section 2i) without a GPU: exported names and
signatures, wholememory_ext_quantized_row_bytes, every argument check of the two entry points through handle-less tensors
under the CPU test backend (no such kernels there: a well-formed call is NOT_SUPPORTED and the counter stays 0; a
malformed one gets its code before that), the Python-side errors, and the numpy restatement of the row format against the
error bound that follows from its roundings."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wholememory_ext_quantized_row_bytes", "wholememory_ext_gather_dequantize", "wholememory_ext_quantize_scatter",
       "wholememory_ext_gather_dequantize_calls")
F32 = np.float32


# ---------------------------------------------------------------- the row format of section 2i, restated
def quantize_ref(x):
    """uint8 [n, round_up(dim, 4) + 8]: every operation one float32 operation of numpy, rounded on its own"""
    x = np.ascontiguousarray(x, F32)
    n, dim = x.shape
    q = (dim + 3) // 4 * 4
    lo = x.min(axis=1) + F32(0.0)   # (a zero minimum is stored as +0.0)
    hi = x.max(axis=1)
    r = hi - lo
    const = r == 0
    safe = np.where(const, F32(1.0), r)
    scale = np.where(const, F32(1.0), safe / F32(255.0)).astype(F32)
    inv = np.where(const, F32(1.0), F32(255.0) / safe).astype(F32)
    codes = np.clip(np.rint((x - lo[:, None]) * inv[:, None]), F32(0.0), F32(255.0)).astype(np.uint8)
    raw = np.zeros((n, q + 8), np.uint8)
    raw[:, :dim] = codes
    raw[:, q:q + 4] = scale.view(np.uint8).reshape(n, 4)
    raw[:, q + 4:q + 8] = lo.astype(F32).view(np.uint8).reshape(n, 4)
    return raw


def dequantize_ref(raw, dim):
    """float32 [n, dim] from uint8 rows: a multiply, then an add"""
    raw = np.ascontiguousarray(raw).view(np.uint8)
    q = (dim + 3) // 4 * 4
    scale = np.ascontiguousarray(raw[:, q:q + 4]).view(F32)
    bias = np.ascontiguousarray(raw[:, q + 4:q + 8]).view(F32)
    return (raw[:, :dim].astype(F32) * scale) + bias


GENERATORS = {
    "normal": lambda rng, n, dim: rng.standard_normal((n, dim)),
    "binades": lambda rng, n, dim: rng.standard_normal((n, dim)) * np.exp2(rng.integers(-12, 13, (n, dim))),
    "offset": lambda rng, n, dim: 1000.0 + rng.standard_normal((n, dim)),
    "dim1": lambda rng, n, dim: rng.standard_normal((n, 1)),
    "dim3": lambda rng, n, dim: rng.standard_normal((n, 3)),
}


@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_restatement_meets_the_bound_of_its_roundings(gen):
    """|y - x| <= 0.5 * scale * (1 + 2^-15) + 4 * 2^-24 * max(|lo|, |hi|). The first term is half a step of the code grid,
    which rounding to the nearest code costs, widened by what the rounded inv and the rounded product may move that decision;
    the second is four float32 roundings (x - lo, scale, c * scale, + bias) of values no larger than max(|lo|, |hi|), each
    2^-24 of such a value at the most."""
    rng = np.random.default_rng(sorted(GENERATORS).index(gen))
    x = GENERATORS[gen](rng, 400, 128).astype(F32)
    n, dim = x.shape
    raw = quantize_ref(x)
    q = (dim + 3) // 4 * 4
    assert raw.shape == (n, q + 8) and not raw[:, dim:q].any()
    y = dequantize_ref(raw, dim)
    scale = np.ascontiguousarray(raw[:, q:q + 4]).view(F32).astype(np.float64)
    lo, hi = x.min(axis=1).astype(np.float64), x.max(axis=1).astype(np.float64)
    bound = 0.5 * scale * (1 + 2.0 ** -15) + 4 * 2.0 ** -24 * np.maximum(np.abs(lo), np.abs(hi))[:, None]
    print(gen, "worst |y - x| / bound:", float((np.abs(y.astype(np.float64) - x) / bound).max()))
    assert (np.abs(y.astype(np.float64) - x.astype(np.float64)) <= bound).all()
    moving = x.max(axis=1) > x.min(axis=1)
    codes = raw[:, :dim]
    assert (codes[moving].min(axis=1) == 0).all() and (codes[moving].max(axis=1) == 255).all()
    assert np.array_equal(y.min(axis=1), x.min(axis=1))            # the minimum comes back exactly
    assert np.array_equal(quantize_ref(y)[:, :dim], codes)         # and quantizing again reproduces every code


def test_restatement_on_constant_rows():
    x = np.repeat(np.array([[0.0], [-3.25], [1e30], [-0.0], [7e-42]], F32), 5, axis=1)
    raw = quantize_ref(x)
    assert not raw[:, :8].any()                                                       # codes and padding
    assert np.array_equal(np.ascontiguousarray(raw[:, 8:12]).view(F32)[:, 0], np.ones(5, F32))   # scale 1.0
    y = dequantize_ref(raw, 5)
    assert np.array_equal(y, x)
    assert np.array_equal(y.view(np.uint32)[[0, 1, 2, 4]], x.view(np.uint32)[[0, 1, 2, 4]])
    assert not y.view(np.uint32)[3].any()                                             # -0.0 rows come back as +0.0


# ---------------------------------------------------------------- names
def test_exported_names(wm_lib):
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import quantized
    assert wgth.quantized is quantized and "quantized" in wgth.__all__
    for name in ("WholeMemoryQuantizedTensor", "create_quantized_tensor", "quantized_row_bytes", "quantize_rows",
                 "dequantize_rows"):
        assert getattr(wgth, name) is getattr(quantized, name) and name in wgth.__all__, name
    assert callable(quantized.calls)
    import pylibwholegraph.torch as plw
    assert plw.create_quantized_tensor is quantized.create_quantized_tensor
    header = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    for name in NEW:
        assert hasattr(wm_lib, name), name
        assert name in header, name
    assert header.index("(2h)") < header.index("(2i)") < header.index("(3) testing seam")
    assert header.index("---- (2h)") < header.index("---- (2i)") < header.index("---- (3) testing seam")
    assert isinstance(wm_lib.wholememory_ext_gather_dequantize_calls(), int)


def test_signatures(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    P = inspect.Parameter

    def params(fn):
        return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()]

    pk, ko, no = P.POSITIONAL_OR_KEYWORD, P.KEYWORD_ONLY, P.empty
    assert params(wgth.quantized_row_bytes) == [("dim", no, pk)]
    assert params(wgth.quantize_rows) == [("values", no, pk)]
    assert params(wgth.dequantize_rows) == [("raw", no, pk), ("dim", no, pk), ("dtype", torch.float32, pk)]
    assert params(wgth.create_quantized_tensor) == [("comm", no, pk), ("memory_type", no, pk), ("memory_location", no, pk),
                                                    ("sizes", no, pk), ("row_align", 16, ko)]
    Q = wgth.WholeMemoryQuantizedTensor
    assert params(Q.__init__) == [("self", no, pk), ("storage", no, pk), ("dim", no, pk)]
    assert params(Q.gather) == [("self", no, pk), ("indice", no, pk), ("force_dtype", None, ko)]
    assert params(Q.scatter) == [("self", no, pk), ("values", no, pk), ("indice", no, pk)]
    assert params(Q.get_comm) == [("self", no, pk)]
    assert isinstance(Q.shape, property)


def test_row_bytes(wm_lib):
    import wholegraph_amd.torch as wgth
    for dim, want in ((1, 12), (3, 12), (4, 12), (5, 16), (127, 136), (128, 136), (129, 140)):
        assert wm_lib.wholememory_ext_quantized_row_bytes(dim) == want == wgth.quantized_row_bytes(dim)
    assert wm_lib.wholememory_ext_quantized_row_bytes(0) == -1 and wm_lib.wholememory_ext_quantized_row_bytes(-5) == -1
    with pytest.raises(ValueError):
        wgth.quantized_row_bytes(0)


# ---------------------------------------------------------------- Python-side checks
def test_python_errors(wm_lib):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.tensor import WholeMemoryTensor

    class Storage(WholeMemoryTensor):
        def __init__(self, dtype, shape, stride, offset=0):
            self.wmb_tensor, self._owns = None, False
            self._cached_layout = (dtype, tuple(shape), tuple(stride), offset)

    Q = wgth.WholeMemoryQuantizedTensor
    with pytest.raises(TypeError):
        Q(object(), 4)                                              # not a WholeMemory tensor
    with pytest.raises(TypeError):
        Q(Storage(torch.float32, (10, 16), (16, 1)), 4)             # not int8
    with pytest.raises(ValueError):
        Q(Storage(torch.int8, (160,), (1,)), 4)                     # not 2-D
    with pytest.raises(ValueError):
        Q(Storage(torch.int8, (10, 12), (12, 1)), 5)                # rows too short for dim 5 (16 bytes)
    with pytest.raises(ValueError):
        Q(Storage(torch.int8, (10, 12), (14, 1)), 4)                # row stride no multiple of 4
    with pytest.raises(ValueError):
        Q(Storage(torch.int8, (10, 12), (16, 1), 2), 4)             # storage offset no multiple of 4
    with pytest.raises(ValueError):
        Q(Storage(torch.int8, (10, 12), (16, 1)), 0)
    t = Q(Storage(torch.int8, (10, 12), (16, 1), 32), 3)
    assert t.shape == (10, 3) and t.dim_ == 3 and isinstance(t.storage, WholeMemoryTensor)
    ids = torch.zeros(2, dtype=torch.int64)
    for bad_values in (torch.zeros((2, 3), dtype=torch.float64), torch.zeros((2, 3), dtype=torch.int32), [[0.0] * 3] * 2):
        with pytest.raises(TypeError):
            t.scatter(bad_values, ids)
    with pytest.raises(ValueError):
        t.scatter(torch.zeros((2, 4)), ids)                         # columns
    with pytest.raises(ValueError):
        t.scatter(torch.zeros(6), ids)                              # not 2-D
    with pytest.raises(ValueError):
        t.scatter(torch.zeros((3, 3)), ids)                         # counts
    with pytest.raises(TypeError):
        t.scatter(torch.zeros((2, 3)), ids.to(torch.int16))
    with pytest.raises(ValueError):
        t.scatter(torch.zeros((2, 3)), ids.reshape(1, 2))
    with pytest.raises(TypeError):
        t.gather(ids.to(torch.float32))
    with pytest.raises(ValueError):
        t.gather(ids.reshape(2, 1))
    for bad in (torch.float64, torch.int8):
        with pytest.raises(TypeError):
            t.gather(ids, force_dtype=bad)
        with pytest.raises(TypeError):
            wgth.dequantize_rows(torch.zeros((2, 12), dtype=torch.int8), 3, bad)
    with pytest.raises(TypeError):
        wgth.dequantize_rows(torch.zeros((2, 12), dtype=torch.uint8), 3)
    with pytest.raises(ValueError):
        wgth.dequantize_rows(torch.zeros((2, 12), dtype=torch.int8), 5)
    with pytest.raises(ValueError):
        wgth.dequantize_rows(torch.zeros(24, dtype=torch.int8), 3)
    with pytest.raises(TypeError):
        wgth.quantize_rows(torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        wgth.quantize_rows(torch.zeros(6))
    for bad_align in (0, 6, -4):
        with pytest.raises(ValueError):
            wgth.create_quantized_tensor(None, "chunked", "cuda", [10, 4], row_align=bad_align)
    with pytest.raises(ValueError):
        wgth.create_quantized_tensor(None, "chunked", "cuda", [10], row_align=16)
    with pytest.raises(ValueError):
        wgth.create_quantized_tensor(None, "chunked", "cuda", [10, 0])


# ---------------------------------------------------------------- the C entry points under the CPU test backend
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
env = L.wholememory_get_default_env_func()
buf = (C.c_char * 4096)()
made = []


def tensor(sizes, dtype, strides=None, offset=0, ptr=buf):
    desc = wmb.make_tensor_desc(list(sizes), dtype, strides, offset)
    t = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(t), C.cast(ptr, C.c_void_p) if ptr is not None else None,
                                                     C.byref(desc)))
    made.append(t)
    return t


DIM, N, ROWS = 5, 3, 8          # row_bytes(5) = 16
ok = dict(table=tensor((ROWS, 16), wmb.DT_INT8), dim=DIM, ids=tensor((N,), wmb.DT_INT64), out=tensor((N, DIM), wmb.DT_FLOAT),
          sms=-1)


def gather(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_gather_dequantize(a["table"], a["dim"], a["ids"], a["out"], env, None, a["sms"])


def scatter(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_quantize_scatter(a["out"], a["ids"], a["table"], a["dim"], env, None, a["sms"])


INV, LOGIC, NOSUP = 6, 3, 9
results = []


def expect(what, code, **over):
    for name, fn in (("gather", gather), ("scatter", scatter)):
        got = fn(**over)
        results.append((name + " " + what, got, code))


# well-formed calls: the checks pass, then the backend has no such kernel
expect("ok", NOSUP)
expect("ok int32 ids", NOSUP, ids=tensor((N,), wmb.DT_INT))
expect("ok fewer ids than rows", NOSUP, ids=tensor((2,), wmb.DT_INT64))
expect("ok no ids", NOSUP, ids=None)
expect("ok n = 0", NOSUP, ids=tensor((0,), wmb.DT_INT64))
expect("ok wide rows", NOSUP, table=tensor((ROWS, 20), wmb.DT_INT8, [32, 1]))
expect("ok row-range view", NOSUP, table=tensor((ROWS - 2, 16), wmb.DT_INT8, [16, 1], 32))
expect("ok padded plain", NOSUP, out=tensor((N, DIM), wmb.DT_FLOAT, [9, 1], 3))
expect("ok dim 4 in 12 bytes", NOSUP, table=tensor((ROWS, 12), wmb.DT_INT8), dim=4, out=tensor((N, 4), wmb.DT_FLOAT))
for dt in (wmb.DT_HALF, wmb.DT_BF16):   # outputs of the gather only
    results.append(("gather ok 16-bit output", gather(out=tensor((N, DIM), dt)), NOSUP))
    results.append(("scatter 16-bit input", scatter(out=tensor((N, DIM), dt)), INV))
# malformed ones
expect("null table", INV, table=None)
expect("null plain", INV, out=None)
expect("dim 0", INV, dim=0, out=tensor((N, 1), wmb.DT_FLOAT))
expect("dim -1", INV, dim=-1)
expect("table 1-D", INV, table=tensor((ROWS * 16,), wmb.DT_INT8))
expect("table int32", INV, table=tensor((ROWS, 16), wmb.DT_INT))
expect("table float", INV, table=tensor((ROWS, 16), wmb.DT_FLOAT))
expect("table rows too short", INV, table=tensor((ROWS, 15), wmb.DT_INT8, [16, 1]))
expect("table rows too short for dim", INV, table=tensor((ROWS, 12), wmb.DT_INT8, [16, 1]))
expect("table stride no multiple of 4", INV, table=tensor((ROWS, 16), wmb.DT_INT8, [18, 1]))
expect("table offset no multiple of 4", INV, table=tensor((ROWS, 16), wmb.DT_INT8, [20, 1], 2))
expect("column-offset view", INV, table=tensor((ROWS, 16), wmb.DT_INT8, [24, 1], 24 + 3))
expect("plain 1-D", INV, out=tensor((N * DIM,), wmb.DT_FLOAT))
expect("plain columns", INV, out=tensor((N, DIM + 1), wmb.DT_FLOAT))
expect("plain columns (fewer)", INV, out=tensor((N, DIM - 1), wmb.DT_FLOAT))
expect("plain double", INV, out=tensor((N, DIM), wmb.DT_DOUBLE))
expect("plain int32", LOGIC, out=tensor((N, DIM), wmb.DT_INT))
expect("plain int8", LOGIC, out=tensor((N, DIM), wmb.DT_INT8))
expect("ids 2-D", INV, ids=tensor((N, 1), wmb.DT_INT64))
expect("ids float", INV, ids=tensor((N,), wmb.DT_FLOAT))
expect("ids int16", INV, ids=tensor((N,), wmb.DT_INT16))
expect("more ids than plain rows", INV, ids=tensor((N + 1,), wmb.DT_INT64))
expect("no ids, more plain rows than table rows", INV, ids=None, out=tensor((ROWS + 1, DIM), wmb.DT_FLOAT))
expect("ids without data", INV, ids=tensor((N,), wmb.DT_INT64, ptr=None))
expect("plain without data", INV, out=tensor((N, DIM), wmb.DT_FLOAT, ptr=None))
for what, got, want in results:
    print("CASE", got, want, what)
print("CALLS", L.wholememory_ext_gather_dequantize_calls())
for t in made:
    L.wholememory_destroy_tensor(t)
'''


def test_entry_points_check_their_arguments_under_the_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    cases = [l.split(None, 3) for l in p.stdout.splitlines() if l.startswith("CASE")]
    assert len(cases) >= 2 * 30
    wrong = [(what, int(got), int(want)) for _, got, want, what in cases if got != want]
    assert not wrong, wrong
    from wholegraph_amd import binding
    assert {int(want) for _, _, want, _ in cases} == {binding.NOT_SUPPORTED, 6, 3}
    assert [l for l in p.stdout.splitlines() if l.startswith("CALLS")] == ["CALLS 0"]
