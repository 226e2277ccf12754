"""The random-walk surface without a GPU: the C entry point (declared in section 2m of the extension header, exported,
bound), its argument checks on host tensors wrapped as wholememory tensors — every answer comes before any device work, under
the product backend and under the CPU test backend, which has no walk kernels and answers NOT_SUPPORTED to a well-formed
call — and the names, signatures and Python-side errors of wholegraph_ops.random_walk and GraphStructure.random_walk."""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wholememory_ext_csr_random_walk"
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_symbol_declared_exported_and_bound(wm_lib):
    import ctypes as C
    from wholegraph_amd import binding
    assert binding.ERROR_NAMES[INV] == "WHOLEMEMORY_INVALID_INPUT" and binding.ERROR_NAMES[LOGIC] == "WHOLEMEMORY_LOGIC_ERROR"
    restype, argtypes = binding.PROTOTYPES[NAME]
    assert restype is C.c_int and len(argtypes) == 9
    assert argtypes[4] is C.c_int and argtypes[5] is C.c_ulonglong
    assert all(t is C.c_void_p for i, t in enumerate(argtypes) if i not in (4, 5))
    assert hasattr(wm_lib, NAME)
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())
    with open(os.path.join(ROOT, "wholegraph_amd", "csrc", "exports.map")) as f:
        assert "wholememory_*;" in f.read()


def test_header_states_the_walk_between_2l_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2m)") == 1
    l2, m2, seam = text.index("---- (2l)"), text.index("---- (2m)"), text.index("---- (3) testing seam")
    assert l2 < m2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2m)") == 1 and head.index("(2l)") < head.index("(2m)") < head.index("(3) the testing seam")
    assert text.count(NAME + "(") == 1 and m2 < text.index(NAME + "(") < seam
    section = " ".join(text[m2:seam].replace("\n *", "\n").split())
    for words in ("z += 0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "mix(mix(seed + a) + b)",
                  "subsequence = a, offset = 0", "0xe220a8397b1dcdaf", "2748719185, 1404529248, 2891244060, 1914411027",
                  "2746596618, 1305647937, 1544306493", "stream(seed, w, 0)", "k = (uint64(r) * uint64(deg)) >> 32",
                  "stream(seed, w * L + t, j + 1)", "ties go to the lowest j", "whether or not earlier steps were taken",
                  "is <= 0 or >= 2^31", "outside [0, n_nodes)", "not on the launch geometry and not on n", "NOT_IMPLEMENTED",
                  "NOT_SUPPORTED", "n = 0 succeeds and queues nothing"):
        assert words in section, words


def test_python_names_and_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    import pylibwholegraph.torch as alias
    from wholegraph_amd.torch import wholegraph_ops
    E = inspect.Parameter.empty
    KW, POS = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = inspect.signature(wholegraph_ops.random_walk)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("wm_csr_row_ptr_tensor", E, POS), ("wm_csr_col_ptr_tensor", E, POS), ("start_nodes_tensor", E, POS),
        ("walk_length", E, POS), ("random_seed", None, POS), ("wm_csr_weight_ptr_tensor", None, KW),
        ("need_edge_output", False, KW)]
    sig = inspect.signature(wgth.GraphStructure.random_walk)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("start_nodes", E, POS), ("walk_length", E, POS), ("weight_name", None, KW), ("random_seed", None, KW),
        ("need_edge_ids", False, KW)]
    # exported the way their neighbours are: the module and the class, and through the pylibwholegraph.torch alias
    assert wgth.wholegraph_ops.random_walk is wholegraph_ops.random_walk
    assert alias.wholegraph_ops.random_walk is wholegraph_ops.random_walk
    assert alias.GraphStructure.random_walk is wgth.GraphStructure.random_walk


def test_python_side_errors_come_before_the_library(wm_lib, monkeypatch):
    import torch
    from wholegraph_amd import binding
    from wholegraph_amd.torch import wholegraph_ops
    monkeypatch.setattr(binding, "lib", lambda: pytest.fail("reached the library"))
    starts = torch.zeros(4, dtype=torch.int64)
    for bad in (0, -1, -80):
        with pytest.raises(ValueError, match="walk_length"):
            wholegraph_ops.random_walk(None, None, starts, bad)
    for bad in (starts.reshape(2, 2), starts[0]):
        with pytest.raises(ValueError, match="1-D"):
            wholegraph_ops.random_walk(None, None, bad, 3)
    import types
    import wholegraph_amd.torch as wgth
    g = wgth.GraphStructure()
    g.csr_row_ptr = g.csr_col_ind = types.SimpleNamespace(wmb_tensor=None)
    with pytest.raises(ValueError, match="walk_length"):
        g.random_walk(starts, 0, random_seed=1)
    with pytest.raises(ValueError, match="1-D"):
        g.random_walk(starts.reshape(2, 2), 3)
    with pytest.raises(AssertionError, match="no edge attribute"):
        g.random_walk(starts, 3, weight_name="w")


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
          steps=steps, walks=wrap(np.zeros((n, steps + 1), i64)), eids=wrap(np.zeros((n, steps), i64)))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_random_walk(a["row"], a["col"], a["wgt"], a["starts"], a["steps"], C.c_ulonglong(7), a["walks"],
                                             a["eids"], None)
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
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [call(), call(eids=None), call(wgt=wrap(np.ones(n_edges, f32))), call(wgt=wrap(np.ones(n_edges, f64)), eids=None),
            call(walks=wrap(np.zeros(n * (steps + 1), i64)), eids=wrap(np.zeros(n * steps, i64))),
            call(starts=wrap(np.zeros(0, i64)), walks=wrap(np.zeros((0, steps + 1), i64)), eids=None)]
print("RESULT", len(invalid), len(logic), *invalid, *logic, *good)
'''


def _child(backend):
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, backend], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    a, b, *codes = (int(v) for v in line.split()[1:])
    return codes[:a], codes[a:a + b], codes[a + b:]


def test_argument_checks_and_not_supported_under_the_cpu_test_backend(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    from wholegraph_amd import binding
    invalid, logic, good = _child("oracle")
    assert len(invalid) == 16 and invalid == [INV] * 16        # (the argument checks come first, whatever the backend)
    assert len(logic) == 9 and logic == [LOGIC] * 9
    assert good == [binding.NOT_SUPPORTED] * 6                  # no walk kernels in that backend: nothing queued


def test_argument_checks_under_the_product_backend(wm_lib):
    """the same malformed calls with the product's backend installed and no device: answered before any device work"""
    invalid, logic, good = _child("hip")
    assert invalid == [INV] * 16 and logic == [LOGIC] * 9 and good == []
