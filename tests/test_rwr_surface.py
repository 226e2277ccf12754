"""The importance-neighbourhood surface without a GPU: the C entry point (section 2s of the extension header, exported, bound),
its argument checks on wrapped host tensors under both backends, and the signatures of the Python entry points."""
import inspect
import os
import subprocess
import sys

from test_neg_surface import _CHILD as _NEG_CHILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wholememory_ext_csr_rwr_top_neighbors"
INV, LOGIC = 6, 3   # WHOLEMEMORY_INVALID_INPUT, WHOLEMEMORY_LOGIC_ERROR


def test_symbol_declared_in_2s_exported_and_bound(wm_lib):
    import ctypes as C
    from wholegraph_amd import binding
    restype, argtypes = binding.PROTOTYPES[NAME]
    assert restype is C.c_int and [t for t in argtypes] == [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_double, C.c_int,
                                                                              C.c_ulonglong] + [C.c_void_p] * 3
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH]).decode()
    assert hasattr(wm_lib, NAME) and any(line.split()[-1] == NAME and " T " in line for line in out.splitlines())
    text = open(os.path.join(ROOT, "include", "wholememory", "wholegraph_amd_ext.h")).read()
    r2, s2, seam = text.index("---- (2r)"), text.index("---- (2s)"), text.index("---- (3) testing seam")
    head = text[:text.index("#ifndef")]
    assert text.count("---- (2s)") == 1 and r2 < s2 < seam and head.count("(2s)") == 1 and head.index("(2r)") < head.index("(2s)")
    assert text.count(NAME + "(") == 1 and s2 < text.index(NAME + "(") < seam
    declaration = " ".join(text[text.index(NAME + "("):seam].split(";")[0].split()).replace("wholememory_tensor_t ", "T ")
    assert declaration == NAME + ("(T wm_csr_row_ptr_tensor, T wm_csr_col_ptr_tensor, T seed_nodes_tensor, int num_walks, int walk_length, "
                                  "double restart_prob, int num_neighbors, unsigned long long random_seed, T output_nodes_tensor, "
                                  "T output_counts_tensor, void* stream)"), declaration


def test_python_names_and_signatures(wm_lib):
    import wholegraph_amd.torch as wgth
    import pylibwholegraph.torch as alias
    from wholegraph_amd.torch import wholegraph_ops
    E, KW, POS = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD

    def params(f, skip=1):
        return [(p.name, p.default, p.kind) for p in list(inspect.signature(f).parameters.values())[skip:]]
    walk = [("num_walks", E, KW), ("walk_length", E, KW), ("restart_prob", 0.5, KW)]
    assert params(wholegraph_ops.rwr_top_neighbors, 0) == [
        ("wm_csr_row_ptr_tensor", E, POS), ("wm_csr_col_ptr_tensor", E, POS), ("seed_nodes_tensor", E, POS), ("num_walks", E, POS),
        ("walk_length", E, POS), ("restart_prob", E, POS), ("num_neighbors", E, POS), ("random_seed", None, POS)]
    G, top, seed = wgth.GraphStructure, ("num_neighbors", E, POS), ("random_seed", None, KW)
    assert params(G.pinsage_neighbors) == [("seed_nodes", E, POS), top] + walk + [seed]
    assert params(G.pinsage_sample_one_hop) == [("center_nodes", E, POS), top] + walk + [seed, ("need_center_local_output", False, KW)]
    assert params(G.multilayer_pinsage_sample) == [("node_ids", E, POS), top] + walk + [("random_seeds", None, KW)]
    assert alias.wholegraph_ops.rwr_top_neighbors is wholegraph_ops.rwr_top_neighbors
    assert alias.PinSAGEModel is wgth.pinsage.PinSAGEModel and "PinSAGEModel" in wgth.__all__ and "pinsage" in wgth.__all__


# the child of tests/test_neg_surface.py up to its own arrays (library, backend by argv[2], DT, wrap(a, shape=None)), then ours
_CHILD = _NEG_CHILD[:_NEG_CHILD.index("n_nodes, n_edges")] + r'''
n_nodes, n_edges, n, T = 5, 7, 4, 3
i64, i32, f32 = np.int64, np.int32, np.float32
ok = dict(row=wrap(np.zeros(n_nodes + 1, i64)), col=wrap(np.zeros(n_edges, i64)), seeds=wrap(np.zeros(n, i64)), R=16, L=4, p=0.5,
          T=T, nodes=wrap(np.zeros((n, T), i64)), counts=wrap(np.zeros((n, T), i32)))
def call(**over):
    a = dict(ok, **over)
    return L.wholememory_ext_csr_rwr_top_neighbors(a["row"], a["col"], a["seeds"], a["R"], a["L"], C.c_double(a["p"]), a["T"],
                                                   C.c_ulonglong(7), a["nodes"], a["counts"], None)
big, one = wrap(np.zeros(1, i64), [1 << 29]), wrap(np.zeros(1, i64))      # (2^29 seeds described over one entry: refused unread)
invalid = [call(row=None), call(col=None), call(seeds=None), call(nodes=None), call(counts=None),
           call(row=wrap(np.zeros((2, 3), i64))), call(seeds=wrap(np.zeros((2, 2), i64))),
           call(R=0), call(L=0), call(R=-1), call(R=2049, L=1), call(R=683, L=3), call(T=0), call(T=65), call(p=1.0), call(p=-0.1),
           call(p=float("nan")), call(seeds=big, R=4, T=1, nodes=one, counts=one), call(seeds=big, R=1, T=4, nodes=one, counts=one),
           call(nodes=wrap(np.zeros((n, T + 1), i64))), call(counts=wrap(np.zeros((n + 1, T), i32))),
           call(nodes=wrap(np.zeros(n * T - 1, i64)))]
logic = [call(row=wrap(np.zeros(n_nodes + 1, i32))), call(col=wrap(np.zeros(n_edges, f32))), call(seeds=wrap(np.zeros(n, f32))),
         call(nodes=wrap(np.zeros((n, T), i32))), call(col=wrap(np.zeros(n_edges, i32))), call(counts=wrap(np.zeros((n, T), i64)))]
good = []
if sys.argv[2] == "oracle":   # (under the product backend a well-formed call would reach the device)
    good = [call(), call(R=2048, L=1, p=0.0, T=64, nodes=wrap(np.zeros((n, 64), i64)), counts=wrap(np.zeros(n * 64, i32))),
            call(seeds=wrap(np.zeros(0, i32)), nodes=wrap(np.zeros((0, T), i64)), counts=wrap(np.zeros((0, T), i32)))]
print("RESULT", len(invalid), len(logic), *invalid, *logic, *good)
'''


def _child(backend):
    env = dict(os.environ, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, backend], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    a, b, *codes = (int(v) for v in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:])
    return codes[:a], codes[a:a + b], codes[a + b:]


def test_argument_checks_under_both_backends(wm_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    from wholegraph_amd import binding
    invalid, logic, good = _child("oracle")
    assert len(invalid) == 22 and invalid == [INV] * 22        # (the argument checks come first, whatever the backend)
    assert len(logic) == 6 and logic == [LOGIC] * 6
    assert good == [binding.NOT_SUPPORTED] * 3                  # no such kernel in that backend: nothing queued
    assert _child("hip") == ([INV] * 22, [LOGIC] * 6, [])      # the product backend, no device: before any device work
