"""The step rule of a node2vec walk (include/wholememory/wholegraph_amd_ext.h section 2n) without a GPU: the bias, the effective
weight and both membership searches live in csrc/walk_n2v.hpp, which compiles for the host. tests/cpp/n2v_walk_test.cpp
includes that header and csrc/pcg.hpp alone, is built here with the host compiler's address and undefined-behaviour sanitizers
(and -ffp-contract=off, as the library is) and run as a process of its own; the walks it prints are compared, bit for bit, with
tests/_n2v_ref.py, the definition restated in Python. Nothing is loaded into this interpreter but the oracle. Also here, because
they are conditions on the definition itself: the lower bounds that keep the cases of the GPU test's graph populated, and the
chi-square values of the kite, which the kernel must reproduce exactly."""
import os
import re
import subprocess

import numpy as np
import pytest

import _n2v_ref as ref
import _walk_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTH, SEED = 5, 0xC0FFEE1234567


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("n2v_walk") / "n2v_walk_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "n2v_walk_test.cpp"), "-o", exe],
                        capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    return exe


def run(program, tmp_path, graph, length, seed, p, q, weights, route):
    """weights: None, or a float32 / float64 array; route 0 scans, 1 searches -> walks, edge ids"""
    row_ptr, col, starts = graph
    kind = 0 if weights is None else 1 if weights.dtype == np.float32 else 2
    numbers = [row_ptr.shape[0] - 1, col.shape[0], starts.shape[0], length, seed,
               int(np.float32(p).view(np.uint32)), int(np.float32(q).view(np.uint32)), kind, route]
    numbers += list(row_ptr) + list(col)
    if kind:
        numbers += list(weights.view(np.uint32 if kind == 1 else np.uint64))
    numbers += list(starts)
    path = tmp_path / "graph.txt"
    path.write_text(" ".join(str(int(x)) for x in numbers) + "\n")
    out = subprocess.run([program, str(path)], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-4000:])
    walks, eids = [], []
    for w, line in enumerate(out.stdout.decode().splitlines()):
        head, _, rest = line.partition(":")
        assert head.split() == ["N", str(w)]
        nodes, _, edges = rest.partition("|")
        walks.append([int(x) for x in nodes.split()])
        eids.append([int(x) for x in edges.split()])
    assert len(walks) == starts.shape[0]
    return np.array(walks, dtype=np.int64).reshape(-1, length + 1), np.array(eids, dtype=np.int64).reshape(-1, length)


def small_graphs():
    """the graph of tests/test_walk_streams.py — 60 nodes of up to 9 neighbours, a hub of 300 that a quarter of the entries
    point at (so that triangles and ways back abound), a node without edges, col_ind entries of -1, n_nodes and 2^31 - 1,
    weights with zeros, negatives, a NaN and -0.0 — with every row ascending (the damaged entries sorted with the rest, the
    weights carried along), and the same rows shuffled -> (sorted form, shuffled form), each row_ptr, col, weights, starts"""
    from test_walk_streams import small_graph
    row_ptr, col, weights, starts = small_graph()
    col, weights = np.array(col), np.array(weights)
    ref._sort_rows(row_ptr, col, weights)
    rng = np.random.default_rng(3)
    mixed_col, mixed_weights = np.array(col), np.array(weights)
    for v in range(row_ptr.shape[0] - 1):
        s, e = int(row_ptr[v]), int(row_ptr[v + 1])
        o = rng.permutation(e - s)
        mixed_col[s:e], mixed_weights[s:e] = col[s:e][o], weights[s:e][o]
    assert not np.array_equal(col, mixed_col)
    assert {-1, 60, (1 << 31) - 1} <= set(col.tolist()) and np.isnan(weights).any() and (weights < 0).any()
    return (row_ptr, col, weights, starts), (row_ptr, mixed_col, mixed_weights, starts)


@pytest.mark.parametrize("kind", ["none", "float", "double"])
def test_walks_of_the_header_equal_the_restated_definition(program, tmp_path, kind):
    in_order, shuffled = small_graphs()
    classes = {"returns": 0, "near": 0, "far": 0}
    for p, q in ref.PQ:
        for name, (row_ptr, col, w32, starts), routes in (("sorted", in_order, (0, 1)), ("shuffled", shuffled, (0,))):
            weights = None if kind == "none" else w32 if kind == "float" else w32.astype(np.float64)
            want = ref.node2vec_walks(row_ptr, col, weights, starts, LENGTH, p, q, SEED)
            for route in routes:
                got = run(program, tmp_path, (row_ptr, col, starts), LENGTH, SEED, p, q, weights, route)
                what = "%s rows, route %d, p = %g, q = %g, weights %s" % (name, route, p, q, kind)
                assert np.array_equal(got[0], want[0]), "walks differ: " + what
                assert np.array_equal(got[1], want[1]), "edge ids differ: " + what
            walks, eids = want
            assert np.array_equal(col[eids[eids >= 0]], walks[:, 1:][eids >= 0]) and (eids < 0).any()
            if (p, q) == (1.0, 1.0):      # the first-order walk: over the weights, or over a tensor of ones
                ones = np.ones(col.shape[0], dtype=np.float32)
                plain = wref.weighted_walks(row_ptr, col, ones if weights is None else weights, starts, LENGTH, SEED)
                assert np.array_equal(walks, plain[0]) and np.array_equal(eids, plain[1]), what
            elif name == "sorted":
                for w in range(walks.shape[0]):
                    for t in range(1, LENGTH):
                        if eids[w, t] < 0:
                            break
                        u, x = int(walks[w, t - 1]), int(walks[w, t + 1])
                        near = col[row_ptr[u]:row_ptr[u + 1]]
                        classes["returns" if x == u else "near" if x in near else "far"] += 1
    print("steps t >= 1 of the sorted form by class: %s" % classes)
    assert min(classes.values()) >= 20, classes


def test_searches_stay_inside_the_row_whatever_it_holds(program, tmp_path):
    """a broken col_sorted promise: the binary search over shuffled rows (the program reads col_ind through a checked
    accessor and runs under the address sanitizer) ends normally, and every step it takes follows an edge of the current node"""
    row_ptr, col, weights, starts = small_graphs()[1]
    walks, eids = run(program, tmp_path, (row_ptr, col, starts), LENGTH, SEED, 0.25, 4.0, weights, 1)
    taken = eids >= 0
    assert taken.sum() >= 50 and np.array_equal(col[eids[taken]], walks[:, 1:][taken])
    src = walks[:, :-1][taken]
    assert ((eids[taken] >= row_ptr[src]) & (eids[taken] < row_ptr[src + 1])).all()


def test_clustered_ladder_reference_holds_its_cases():
    """the lower bounds tests/test_n2v_gpu.py relies on, on the reference walks of the clustered ladder (no GPU needed to know
    that the graph exercises its cases); the unsorted twin holds the same rows"""
    measures = ref.assert_ladder_measures()
    print("clustered ladder measures: %s" % measures)
    row_ptr, col, weights, _ = ref.clustered_ladder()
    assert all((np.diff(col[row_ptr[v]:row_ptr[v + 1]]) >= 0).all() for v in range(ref.NODES)), "a row is not ascending"
    t_ptr, t_col, t_weights, _ = ref.unsorted_twin()
    assert int(np.diff(t_ptr).max()) == ref.TWIN_CAP
    unsorted = 0
    for v in range(ref.NODES):
        s, e, ts, te = int(row_ptr[v]), int(row_ptr[v + 1]), int(t_ptr[v]), int(t_ptr[v + 1])
        o = np.lexsort((t_weights[ts:te], t_col[ts:te]))
        head = np.lexsort((weights[s:s + te - ts], col[s:s + te - ts]))
        assert np.array_equal(t_col[ts:te][o], col[s:s + te - ts][head])
        assert np.array_equal(t_weights[ts:te][o], weights[s:s + te - ts][head])
        unsorted += int((np.diff(t_col[ts:te]) < 0).any())
    assert unsorted >= 1000


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_kite_walks_follow_the_biases(program, tmp_path, weighted):
    """24 000 walks 1 -> ? -> ? on the kite; among those through node 0 the second step follows {1: 1 / p; 2, 3: 1; 4, 5, 6:
    1 / q} (times the weights): chi-square over 5 degrees of freedom below 40, the samplers' bar. The value is recorded (here
    and in DESIGN.md 3.18): the kernel walks the same walks, so tests/test_n2v_gpu.py asks for exactly this value."""
    row_ptr, col, weights = ref.kite()
    starts = np.ones(ref.KITE_WALKS, dtype=np.int64)
    walks, _ = run(program, tmp_path, (row_ptr, col, starts), ref.KITE_LENGTH, ref.KITE_SEED, ref.KITE_P, ref.KITE_Q,
                   weights if weighted else None, 1)
    chi2 = ref.kite_statistic(walks, weighted)
    print("kite, %s: chi-square %.4f over 5 dof" % ("weighted" if weighted else "unweighted", chi2))
    assert chi2 < 40.0
    assert abs(chi2 - ref.KITE_CHI2[weighted]) < 1e-6, (chi2, ref.KITE_CHI2[weighted])
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        section = f.read().split("### 3.18")[1].split("\n## ")[0]
    assert re.search(r"\b%.4f\b" % ref.KITE_CHI2[weighted], section), "DESIGN.md 3.18 does not state %.4f" % ref.KITE_CHI2[weighted]
