"""The negative-sampling surface without a GPU: the C entry point (declared in section 2o of the extension header, exported,
bound), its argument checks on host tensors wrapped as wholememory tensors — every answer before any device work, under the
product backend and under the CPU test backend, which has no such kernel and answers NOT_SUPPORTED to a well-formed call; and
the names, signatures and Python-side errors of wholegraph_ops.negative_sample and GraphStructure.negative_sample."""
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wholememory_ext_csr_negative_sample"
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_symbol_declared_exported_and_bound(wm_lib):
    import ctypes as C
    from wholegraph_amd import binding
    restype, argtypes = binding.PROTOTYPES[NAME]
    assert restype is C.c_int and len(argtypes) == 11
    assert all(argtypes[i] is C.c_int for i in (3, 4, 5, 6, 7)) and argtypes[8] is C.c_ulonglong
    assert all(argtypes[i] is C.c_void_p for i in (0, 1, 2, 9, 10))
    assert hasattr(wm_lib, NAME)
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    assert any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())


def test_header_states_the_op_between_2n_and_the_testing_seam():
    with open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")) as f:
        text = f.read()
    assert text.count("---- (2o)") == 1
    n2, o2, seam = text.index("---- (2n)"), text.index("---- (2o)"), text.index("---- (3) testing seam")
    assert n2 < o2 < seam
    head = text[:text.index("#ifndef")]
    assert head.count("(2o)") == 1 and head.index("(2n)") < head.index("(2o)") < head.index("(3) the testing seam")
    assert text.count(NAME + "(") == 1 and o2 < text.index(NAME + "(") < seam
    declaration = " ".join(re.sub(r"/\*.*?\*/", " ", text[text.index(NAME + "("):seam].split(";")[0]).split())   # (without comments)
    assert declaration == (NAME + "(wholememory_tensor_t wm_csr_row_ptr_tensor, wholememory_tensor_t wm_csr_col_ptr_tensor, "
                           "wholememory_tensor_t src_nodes_tensor, int num_negatives, int mode, int exclude, int max_tries, "
                           "int col_sorted, unsigned long long random_seed, wholememory_tensor_t output_negatives_tensor, "
                           "void* stream)"), declaration
    section = " ".join(text[o2:seam].replace("\n *", "\n").split())
    for words in ("as (2m)", "given as 2-D or as 1-D with n * K entries", "does not synchronise",
                  "stream(seed, i * K + k, 0)", "low word first", "pcg32::next_u64",
                  "whether or not earlier attempts were rejected", "c = (r * n_nodes) >> 64, a 128-bit product",
                  "pos = (r * n_edges) >> 64 and c = col_ind[pos]", "With n_edges = 0 every attempt is rejected",
                  "c is outside [0, n_nodes)", "exclude & 2 is set and c == u",
                  "exclude & 1 is set and c occurs in col_ind[row_ptr[u] : row_ptr[u + 1]]",
                  "if all T attempts are rejected the output is -1", "when u is outside [0, n_nodes)",
                  "0 <= s <= e <= n_edges and e - s < 2^31", "drawn with replacement",
                  "every row of col_ind is ascending", "binary search", "the class of a candidate is not specified",
                  "Only ids are compared", "never used as an index before it is range-checked",
                  "depends on (seed, i, k, a), K and the graph only", "not on which search route answered",
                  "max_tries outside [1, 64]", "exclude outside [0, 3]", "n * K >= 2^31", "HIERARCHY",
                  "NOT_IMPLEMENTED", "NOT_SUPPORTED", "n = 0 succeeds and queues nothing"):
        assert words in section, words


def test_python_names_and_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    import pylibwholegraph.torch as alias
    from wholegraph_amd.torch import wholegraph_ops
    E = inspect.Parameter.empty
    KW, POS = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    sig = inspect.signature(wholegraph_ops.negative_sample)
    assert [(p.name, p.default, p.kind) for p in sig.parameters.values()] == [
        ("wm_csr_row_ptr_tensor", E, POS), ("wm_csr_col_ptr_tensor", E, POS), ("src_nodes_tensor", E, POS),
        ("num_negatives", E, POS), ("random_seed", None, POS), ("mode", "uniform", KW), ("exclude_edges", True, KW),
        ("exclude_self", True, KW), ("max_tries", 8, KW), ("col_sorted", False, KW)]
    sig = inspect.signature(wgth.GraphStructure.negative_sample)
    assert [(p.name, p.default, p.kind) for p in list(sig.parameters.values())[1:]] == [
        ("src_nodes", E, POS), ("num_negatives", E, POS), ("mode", "uniform", KW), ("exclude_edges", True, KW),
        ("exclude_self", True, KW), ("max_tries", 8, KW), ("random_seed", None, KW), ("col_sorted", False, KW)]
    # exported the way random_walk is: the module and the class, and through the pylibwholegraph.torch alias
    assert wgth.wholegraph_ops.negative_sample is wholegraph_ops.negative_sample
    assert alias.wholegraph_ops.negative_sample is wholegraph_ops.negative_sample
    assert alias.GraphStructure.negative_sample is wgth.GraphStructure.negative_sample


def test_python_side_errors_come_before_the_library(wm_lib, monkeypatch):
    import torch
    from wholegraph_amd import binding
    from wholegraph_amd.torch import wholegraph_ops
    monkeypatch.setattr(binding, "lib", lambda: pytest.fail("reached the library"))
    src = torch.zeros(4, dtype=torch.int64)
    for bad in (0, -1, -5):
        with pytest.raises(ValueError, match="num_negatives"):
            wholegraph_ops.negative_sample(None, None, src, bad)
    for bad in (0, -1, 65, 1000):
        with pytest.raises(ValueError, match="max_tries"):
            wholegraph_ops.negative_sample(None, None, src, 5, max_tries=bad)
    for bad in ("", "Uniform", "by_degree", 0, None):
        with pytest.raises(ValueError, match="mode"):
            wholegraph_ops.negative_sample(None, None, src, 5, mode=bad)
    for bad in (src.reshape(2, 2), src[0]):
        with pytest.raises(ValueError, match="1-D"):
            wholegraph_ops.negative_sample(None, None, bad, 5)
    import types
    import wholegraph_amd.torch as wgth
    g = wgth.GraphStructure()
    g.csr_row_ptr = g.csr_col_ind = types.SimpleNamespace(wmb_tensor=None)
    with pytest.raises(ValueError, match="num_negatives"):
        g.negative_sample(src, 0, random_seed=1)
    with pytest.raises(ValueError, match="max_tries"):
        g.negative_sample(src, 5, max_tries=65, col_sorted=True)
    with pytest.raises(ValueError, match="mode"):
        g.negative_sample(src, 5, mode="alias")
    with pytest.raises(ValueError, match="1-D"):
        g.negative_sample(src.reshape(2, 2), 5, exclude_self=False)


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
      np.dtype(np.int16): wmb.DT_INT16}
keep = []
def wrap(a, shape=None):
    """a host array as a wholememory tensor (nothing here reaches the point where its memory would be read); shape: what the
    description claims, whatever the array holds"""
    a = np.ascontiguousarray(a)
    keep.append(a)
    desc = wmb.make_tensor_desc(list(a.shape if shape is None else shape), DT[a.dtype])
    h = C.c_void_p()
    wmb.check(L.wholememory_make_tensor_from_pointer(C.byref(h), C.c_void_p(a.ctypes.data), C.byref(desc)))
    return h
n_nodes, n_edges, n, K = 5, 7, 4, 3
i64, i32, f32 = np.int64, np.int32, np.float32
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), src=wrap(np.zeros(n, i64)), K=K, mode=0,
          exclude=3, tries=8, srt=0, out=wrap(np.zeros((n, K), i64)))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_negative_sample(a["row"], a["col"], a["src"], a["K"], a["mode"], a["exclude"], a["tries"],
                                                 a["srt"], C.c_ulonglong(7), a["out"], None)
big = 1 << 29      # (a description of 2^29 sources over a one-entry array: refused before anything is read)
invalid = [call(row=None), call(col=None), call(src=None), call(out=None),
           call(row=wrap(np.zeros((2, 3), i64))), call(col=wrap(np.zeros((7, 1), i64))), call(src=wrap(np.zeros((2, 2), i64))),
           call(K=0), call(K=-3), call(tries=0), call(tries=-1), call(tries=65), call(mode=2), call(mode=-1),
           call(exclude=4), call(exclude=-1),
           call(src=wrap(np.zeros(1, i64), [big]), K=4, out=wrap(np.zeros(1, i64))),          # n * K = 2^31
           call(src=wrap(np.zeros(1, i64), [big]), K=(1 << 31) - 1, out=wrap(np.zeros(1, i64))),
           call(out=wrap(np.zeros((n, K + 1), i64))), call(out=wrap(np.zeros((n + 1, K), i64))),
           call(out=wrap(np.zeros((K, n), i64))), call(out=wrap(np.zeros(n * K - 1, i64))),
           call(out=wrap(np.zeros((n, K, 1), i64)))]
logic = [call(row=wrap(np.zeros(n_nodes + 1, i32))), call(col=wrap(np.zeros(n_edges, f32))),
         call(col=wrap(np.zeros(n_edges, np.int16)), out=wrap(np.zeros((n, K), np.int16))),
         call(src=wrap(np.zeros(n, f32))), call(src=wrap(np.zeros(n, np.int16))),
         call(out=wrap(np.zeros((n, K), i32))),
         call(col=wrap(np.zeros(n_edges, i32)))]                                        # output int64 over an int32 col_ind
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [call(), call(srt=1), call(mode=1), call(exclude=0), call(tries=1), call(tries=64), call(K=1, out=wrap(np.zeros((n, 1), i64))),
            call(out=wrap(np.zeros(n * K, i64))), call(src=wrap(np.zeros(n, i32))),
            call(col=wrap(np.zeros(n_edges, i32)), out=wrap(np.zeros((n, K), i32))),
            call(col=wrap(np.zeros(0, i64)), mode=1),
            call(src=wrap(np.zeros(0, i64)), out=wrap(np.zeros((0, K), i64)))]
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
    assert len(invalid) == 23 and invalid == [INV] * 23        # (the argument checks come first, whatever the backend)
    assert len(logic) == 7 and logic == [LOGIC] * 7
    assert good == [binding.NOT_SUPPORTED] * 12                 # no such kernel in that backend: nothing queued


def test_argument_checks_under_the_product_backend(wm_lib):
    """the same malformed calls with the product's backend installed and no device: answered before any device work"""
    invalid, logic, good = _child("hip")
    assert invalid == [INV] * 23 and logic == [LOGIC] * 7 and good == []
