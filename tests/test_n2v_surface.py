"""The node2vec-walk surface without a GPU: the C entry point (declared in section 2n of the extension header, exported,
bound), its argument checks on host tensors wrapped as wholememory tensors — the malformed calls of
tests/test_walk_surface.py again, and p and q — every answer before any device work, under the product backend and under the
CPU test backend, which has no such kernel and answers NOT_SUPPORTED to a well-formed call; and the names, signatures and
Python-side errors of wholegraph_ops.node2vec_walk and GraphStructure.node2vec_walk."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wholememory_ext_csr_node2vec_walk"
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_symbol_declared_exported_and_bound(wm_lib):
    import ctypes as C
    from wholegraph_amd import binding
    restype, argtypes = binding.PROTOTYPES[NAME]
    assert restype is C.c_int and len(argtypes) == 12
    assert argtypes[4] is C.c_int and argtypes[5] is C.c_float and argtypes[6] is C.c_float and argtypes[7] is C.c_int
    assert argtypes[8] is C.c_ulonglong
    assert all(t is C.c_void_p for i, t in enumerate(argtypes) if i not in (4, 5, 6, 7, 8))
    assert hasattr(wm_lib, NAME)
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())


def test_header_states_the_walk_between_2m_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2n)") == 1
    m2, n2, seam = text.index("---- (2m)"), text.index("---- (2n)"), text.index("---- (3) testing seam")
    assert m2 < n2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2n)") == 1 and head.index("(2m)") < head.index("(2n)") < head.index("(3) the testing seam")
    assert text.count(NAME + "(") == 1 and n2 < text.index(NAME + "(") < seam
    declaration = " ".join(text[text.index(NAME + "("):seam].split(";")[0].split())
    for words in ("int walk_length, float p, float q, int col_sorted, unsigned long long random_seed,",):
        assert words in declaration, declaration
    section = " ".join(text[n2:seam].replace("\n *", "\n").split())
    for words in ("as (2m)", "inv_p = 1.0f / p and inv_q = 1.0f / q, one fp32 division each, done on the host",
                  "u = walks[w, t - 1]", "1.0f at t = 0", "inv_p when x == u",
                  "x occurs in col_ind[row_ptr[u] : row_ptr[u + 1]]", "else inv_q", "Only ids are compared",
                  "never used as an index before it is chosen and range-checked", "ew = w32 * a, a single fp32 multiply",
                  "eligible when ew > 0", "stream(seed, w * L + t, j + 1)", "ties go to the lowest j",
                  "With p = q = 1, ew == w32 bit for bit", "equal wholememory_ext_csr_random_walk with the same weight tensor",
                  "weight tensor of ones", "not on which search route answered", "every row of col_ind is ascending",
                  "binary search", "the class of a neighbour is not specified", "1.0f / q are all finite and > 0",
                  "NOT_IMPLEMENTED", "NOT_SUPPORTED", "n = 0 succeeds and queues nothing"):
        assert words in section, words


def test_python_names_and_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    import pylibwholegraph.torch as alias
    from wholegraph_amd.torch import wholegraph_ops
    E = inspect.Parameter.empty
    KW, POS = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = inspect.signature(wholegraph_ops.node2vec_walk)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("wm_csr_row_ptr_tensor", E, POS), ("wm_csr_col_ptr_tensor", E, POS), ("start_nodes_tensor", E, POS),
        ("walk_length", E, POS), ("p", E, POS), ("q", E, POS), ("random_seed", None, POS),
        ("wm_csr_weight_ptr_tensor", None, KW), ("col_sorted", False, KW), ("need_edge_output", False, KW)]
    sig = inspect.signature(wgth.GraphStructure.node2vec_walk)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("start_nodes", E, POS), ("walk_length", E, POS), ("p", E, POS), ("q", E, POS), ("weight_name", None, KW),
        ("random_seed", None, KW), ("col_sorted", False, KW), ("need_edge_ids", False, KW)]
    # exported the way random_walk is: the module and the class, and through the pylibwholegraph.torch alias
    assert wgth.wholegraph_ops.node2vec_walk is wholegraph_ops.node2vec_walk
    assert alias.wholegraph_ops.node2vec_walk is wholegraph_ops.node2vec_walk
    assert alias.GraphStructure.node2vec_walk is wgth.GraphStructure.node2vec_walk


def test_python_side_errors_come_before_the_library(wm_lib, monkeypatch):
    import torch
    from wholegraph_amd import binding
    from wholegraph_amd.torch import wholegraph_ops
    monkeypatch.setattr(binding, "lib", lambda: pytest.fail("reached the library"))
    starts = torch.zeros(4, dtype=torch.int64)
    for bad in (0, -1, -80):
        with pytest.raises(ValueError, match="walk_length"):
            wholegraph_ops.node2vec_walk(None, None, starts, bad, 1.0, 1.0)
    for bad in (starts.reshape(2, 2), starts[0]):
        with pytest.raises(ValueError, match="1-D"):
            wholegraph_ops.node2vec_walk(None, None, bad, 3, 1.0, 1.0)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="p must be finite and positive"):
            wholegraph_ops.node2vec_walk(None, None, starts, 3, bad, 1.0)
        with pytest.raises(ValueError, match="q must be finite and positive"):
            wholegraph_ops.node2vec_walk(None, None, starts, 3, 1.0, bad)
    import types
    import wholegraph_amd.torch as wgth
    g = wgth.GraphStructure()
    g.csr_row_ptr = g.csr_col_ind = types.SimpleNamespace(wmb_tensor=None)
    with pytest.raises(ValueError, match="walk_length"):
        g.node2vec_walk(starts, 0, 1.0, 1.0, random_seed=1)
    with pytest.raises(ValueError, match="1-D"):
        g.node2vec_walk(starts.reshape(2, 2), 3, 1.0, 1.0)
    with pytest.raises(ValueError, match="q must be finite"):
        g.node2vec_walk(starts, 3, 2.0, 0.0, col_sorted=True)
    with pytest.raises(AssertionError, match="no edge attribute"):
        g.node2vec_walk(starts, 3, 1.0, 1.0, weight_name="w")


_CHILD = r'''
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
os.environ["WHOLEGRAPH_AMD_TESTING"] = "1"
import numpy as np
from wholegraph_amd import binding as wmb
L = wmb.lib()
if sys.argv[2] == "oracle":
    tb = C.CDLL(os.path.join(sys.argv[1], "oracle", "libwm_test_backend.so"))
    tb.wm_test_backend.restype = C.c_void_p
    wmb.check(L.wm_testing_install_backend(C.c_void_p(tb.wm_test_backend())))
    assert L.wholememory_ext_backend_name().startswith(b"oracle-test-backend")
else:
    assert L.wholememory_ext_backend_name() == b"hip-gfx950"
DT = {np.dtype(np.int32): wmb.DT_INT, np.dtype(np.int64): wmb.DT_INT64, np.dtype(np.float32): wmb.DT_FLOAT,
      np.dtype(np.float64): wmb.DT_DOUBLE, np.dtype(np.int16): wmb.DT_INT16}
keep = []
def wrap(a):
    """a host array as a wholememory tensor (nothing here reaches the point where its memory would be read)"""
    a = np.ascontiguousarray(a)
    keep.append(a)
    desc = wmb.make_tensor_desc(list(a.shape), DT[a.dtype])
    h = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(h), C.c_void_p(a.ctypes.data), C.byref(desc)))
    return h
n_nodes, n_edges, n, steps = 5, 7, 4, 3
i64, i32, f32, f64 = np.int64, np.int32, np.float32, np.float64
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), wgt=None, starts=wrap(np.zeros(n, i64)),
          steps=steps, p=0.5, q=2.0, srt=0, walks=wrap(np.zeros((n, steps + 1), i64)), eids=wrap(np.zeros((n, steps), i64)))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_node2vec_walk(a["row"], a["col"], a["wgt"], a["starts"], a["steps"], C.c_float(a["p"]),
                                               C.c_float(a["q"]), a["srt"], C.c_ulonglong(7), a["walks"], a["eids"], None)
# the malformed calls of tests/test_walk_surface.py
invalid = [call(row=None), call(col=None), call(starts=None), call(walks=None), call(steps=0), call(steps=-3),
           call(starts=wrap(np.zeros((2, 2), i64))),                                   # start nodes not 1-D
           call(walks=wrap(np.zeros((n, steps), i64))), call(walks=wrap(np.zeros((n + 1, steps + 1), i64))),
           call(walks=wrap(np.zeros(n * (steps + 1) - 1, i64))), call(eids=wrap(np.zeros((n, steps + 1), i64))),
           call(eids=wrap(np.zeros((n - 1, steps), i64))),
           call(wgt=wrap(np.zeros(n_edges - 1, f32))), call(wgt=wrap(np.zeros(n_edges + 1, f64))),
           call(steps=(1 << 31) // n, walks=wrap(np.zeros(1, i64)), eids=None),        # n * (L + 1) >= 2^31
           call(steps=(1 << 31) - 1, walks=wrap(np.zeros(1, i64)), eids=None)]
logic = [call(row=wrap(np.zeros(n_nodes + 1, i32))), call(col=wrap(np.zeros(n_edges, f32))),
         call(col=wrap(np.zeros(n_edges, np.int16)), walks=wrap(np.zeros((n, steps + 1), np.int16))),
         call(starts=wrap(np.zeros(n, f32))), call(walks=wrap(np.zeros((n, steps + 1), i32))),
         call(col=wrap(np.zeros(n_edges, i32))),                                       # walks int64 over an int32 col_ind
         call(eids=wrap(np.zeros((n, steps), i32))), call(wgt=wrap(np.zeros(n_edges, i64))),
         call(wgt=wrap(np.zeros(n_edges, i32)))]
# p or q that is 0, negative, NaN, inf, or a subnormal whose reciprocal overflows, in an otherwise well-formed call
bad_pq = []
for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
    bad_pq += [call(p=bad), call(q=bad), call(p=bad, srt=1, wgt=wrap(np.ones(n_edges, f32)))]
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [call(), call(eids=None), call(srt=1), call(p=1.0, q=1.0), call(p=1e-38, q=1e38),
            call(wgt=wrap(np.ones(n_edges, f32))), call(wgt=wrap(np.ones(n_edges, f64)), eids=None, srt=1),
            call(walks=wrap(np.zeros(n * (steps + 1), i64)), eids=wrap(np.zeros(n * steps, i64))),
            call(starts=wrap(np.zeros(0, i64)), walks=wrap(np.zeros((0, steps + 1), i64)), eids=None)]
print("RESULT", len(invalid), len(logic), len(bad_pq), *invalid, *logic, *bad_pq, *good)
'''


def _child(backend):
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, backend], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    a, b, c, *codes = (int(v) for v in line.split()[1:])
    return codes[:a], codes[a:a + b], codes[a + b:a + b + c], codes[a + b + c:]


def test_argument_checks_and_not_supported_under_the_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    from wholegraph_amd import binding
    invalid, logic, bad_pq, good = _child("oracle")
    assert len(invalid) == 16 and invalid == [INV] * 16        # (the argument checks come first, whatever the backend)
    assert len(logic) == 9 and logic == [LOGIC] * 9
    assert len(bad_pq) == 15 and bad_pq == [INV] * 15
    assert good == [binding.NOT_SUPPORTED] * 9                  # no such kernel in that backend: nothing queued


def test_argument_checks_under_the_product_backend(wm_lib):
    """the same malformed calls with the product's backend installed and no device: answered before any device work"""
    invalid, logic, bad_pq, good = _child("hip")
    assert invalid == [INV] * 16 and logic == [LOGIC] * 9 and bad_pq == [INV] * 15 and good == []
