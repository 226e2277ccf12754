"""The rule of a negative sample (include/wholememory/wholegraph_amd_ext.h section 2o) without a GPU: the candidate of a 64-bit
draw and the rejection rule live in csrc/neg_sample.hpp, which compiles for the host. tests/cpp/neg_sample_test.cpp includes
that header, csrc/walk_n2v.hpp and csrc/pcg.hpp alone, is built here with the host compiler's address and undefined-behaviour
sanitizers (and -ffp-contract=off, as the library is) and run as a process of its own; the samples it prints are compared, bit
for bit, with tests/_neg_ref.py, the definition restated in Python. Nothing is loaded into this interpreter but the oracle.
Also here, because they are conditions on the definition itself: what the reference outputs must and must not contain, and the
statistics of the dozen, which the kernel must reproduce exactly."""
import os
import re
import subprocess

import numpy as np
import pytest

import _neg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xC0FFEE1234567
DAMAGED = (-1, 60, (1 << 31) - 1)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("neg_sample") / "neg_sample_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "neg_sample_test.cpp"), "-o", exe],
                        capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    return exe


def run(program, tmp_path, graph, num_negatives, mode, exclude, max_tries, route, seed):
    """route 0 scans, 1 searches -> negatives int64 [n, K]"""
    row_ptr, col, src = graph
    numbers = [row_ptr.shape[0] - 1, col.shape[0], src.shape[0], num_negatives, mode, exclude, max_tries, route, seed]
    numbers += list(row_ptr) + list(col) + list(src)
    path = tmp_path / "graph.txt"
    path.write_text(" ".join(str(int(x)) for x in numbers) + "\n")
    out = subprocess.run([program, str(path)], capture_output=True, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-4000:])
    rows = []
    for i, line in enumerate(out.stdout.decode().splitlines()):
        head, _, rest = line.partition(":")
        assert head.split() == ["N", str(i)]
        rows.append([int(x) for x in rest.split()])
    assert len(rows) == src.shape[0]
    return np.array(rows, dtype=np.int64).reshape(-1, num_negatives)


def small_graphs():
    """the sorted and the shuffled form of tests/test_n2v_streams.py::small_graphs — 60 nodes, a hub of 300 (node 3), a node
    without edges (node 4), col_ind entries of -1, n_nodes and 2^31 - 1 — each -> row_ptr, col, sources; the sources hold -1,
    n_nodes, the hub and the node without edges"""
    from test_n2v_streams import small_graphs as forms
    in_order, shuffled = forms()
    src = in_order[3]
    assert {-1, 60, 3, 4} <= set(src.tolist()) and in_order[0][5] == in_order[0][4]
    assert set(DAMAGED) <= set(in_order[1].tolist())
    return (in_order[0], in_order[1], src), (shuffled[0], shuffled[1], src)


@pytest.mark.parametrize("mode", [0, 1], ids=["uniform", "degree"])
def test_samples_of_the_header_equal_the_restated_definition(program, tmp_path, mode):
    in_order, shuffled = small_graphs()
    refused, minus, drawn = {}, 0, 0
    for name, graph, routes in (("sorted", in_order, (0, 1)), ("shuffled", shuffled, (0,))):
        row_ptr, col, src = graph
        for exclude in range(4):
            for tries in ref.TRIES:
                for k in ref.KS:
                    want = ref.negative_samples(row_ptr, col, src, k, mode, exclude, tries, SEED, out_of_range=refused)
                    what = "%s rows, mode %d, exclude %d, T = %d, K = %d" % (name, mode, exclude, tries, k)
                    for route in routes:
                        got = run(program, tmp_path, graph, k, mode, exclude, tries, route, SEED)
                        assert np.array_equal(got, want), "route %d: %s" % (route, what)
                    # on the reference itself: no output is a neighbour (exclude & 1) or the source (exclude & 2)
                    ref.assert_outputs_allowed(want, row_ptr, col, src, exclude, what)
                    minus += int((want == -1).sum())
                    drawn += int((want >= 0).sum())
    print("mode %d: %d samples drawn, %d are -1; candidates refused as out of range: %s" % (mode, drawn, minus, refused))
    assert drawn >= 5000 and minus >= 100
    if mode == 1:      # every damaged value was drawn, and refused, at least once
        assert set(refused) == set(DAMAGED) and min(refused.values()) >= 1, refused
    else:
        assert refused == {}


def test_hub_and_edgeless_sources(program, tmp_path):
    """the hub excludes its 300 entries; the node without edges excludes nothing but itself; a refused source gives -1"""
    row_ptr, col, src = small_graphs()[0]
    want = ref.negative_samples(row_ptr, col, src, 33, 0, 3, 8, SEED)
    where = {int(u): i for i, u in enumerate(src)}
    assert (want[where[-1]] == -1).all() and (want[where[60]] == -1).all()
    hub = set(col[row_ptr[3]:row_ptr[4]].tolist())
    assert len(hub & set(range(60))) >= 20 and not set(want[where[3]].tolist()) & (hub | {3})
    assert (want[where[4]] >= 0).all() and 4 not in want[where[4]]
    only_edges = ref.negative_samples(row_ptr, col, src[where[4]:where[4] + 1], 33, 0, 1, 1, SEED, first_source=where[4])
    assert (only_edges >= 0).all()       # nothing is excluded: the first attempt is kept


def test_searches_stay_inside_the_row_whatever_it_holds(program, tmp_path):
    """a broken col_sorted promise: the binary search over shuffled rows (the program reads col_ind through a checked accessor
    and runs under the address sanitizer) ends normally, and every output is a node or -1, never the source with exclude & 2"""
    row_ptr, col, src = small_graphs()[1]
    for mode in (0, 1):
        out = run(program, tmp_path, (row_ptr, col, src), 33, mode, 3, 8, 1, SEED)
        assert ((out == -1) | ((out >= 0) & (out < 60))).all()
        inside = (src >= 0) & (src < 60)
        assert (out[~inside] == -1).all() and not (out[inside] == src[inside, None]).any()
        assert (out >= 0).sum() >= 1000


def test_ladder_reference_holds_its_cases():
    """the lower bounds tests/test_neg_gpu.py relies on, on the REFERENCE outputs of the ladder and of its sorted copy, so that
    a later change of the graph cannot empty a case: every exclusion changes outputs, samples need a later attempt, the
    5000-neighbour node (one source, 33 samples) leaves samples at -1, the three refused ids give -1"""
    src = ref.ladder()[2]
    for in_order in (False, True):
        for mode in (0, 1):
            free, edges, own, both = (ref.ladder_negatives(in_order, 33, mode, x, 8) for x in range(4))
            assert (free != edges).sum() >= 50 and (edges != both).sum() >= 5 and (free != own).sum() >= 5, (in_order, mode)
            once = ref.ladder_negatives(in_order, 33, mode, 3, 1)
            assert ((once == -1) & (both >= 0)).sum() >= 50, "too few samples need a later attempt"
            assert (both[src == 7] == -1).sum() >= 10, "the 5000-neighbour node rejects too little"
            assert (both[(src < 0) | (src >= 2000)] == -1).all() and ((src < 0) | (src >= 2000)).sum() == 3
            assert (both[src == 12] >= 0).all(), "the node without neighbours excludes only itself"


@pytest.mark.parametrize("mode,tries", sorted(ref.DOZEN_VALUES))
def test_the_dozen_follows_its_distribution(program, tmp_path, mode, tries):
    """3000 x 8 negatives of node 0 of the dozen with exclude = 3: all in 6 .. 11; uniform (mode 0) or in proportion to the
    col_ind counts of 6 .. 11 (mode 1): chi-square over 5 degrees of freedom below 40, the samplers' bar. With 16 tries at
    most 0.1 % of the outputs are -1; with 4 tries in mode 0, where an attempt is rejected with probability 1 / 2, between 5 %
    and 7.5 % (2^-4 = 6.25 %). The values are recorded (here and in DESIGN.md 3.19): the kernel draws the same samples, so
    tests/test_neg_gpu.py asks for exactly these values."""
    row_ptr, col = ref.dozen()
    src = np.zeros(ref.DOZEN_SOURCES, dtype=np.int64)
    values = []
    for route in (0, 1):
        out = run(program, tmp_path, (row_ptr, col, src), ref.DOZEN_K, mode, 3, tries, route, ref.DOZEN_SEED)
        values.append(ref.dozen_statistic(out, mode))
    assert values[0] == values[1]
    share, chi2 = values[0]
    print("the dozen, mode %d, T = %d: %d of %d are -1, chi-square %.4f over 5 dof" % (mode, tries, round(share * out.size),
                                                                                    out.size, chi2))
    assert chi2 < 40.0
    assert share <= 0.001 if tries == 16 else 0.05 <= share <= 0.075
    missing, recorded = ref.DOZEN_VALUES[(mode, tries)]
    assert round(share * out.size) == missing and abs(chi2 - recorded) < 1e-6, (share * out.size, chi2, missing, recorded)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        section = f.read().split("### 3.19")[1].split("\n## ")[0]
    assert re.search(r"\b%.4f\b" % recorded, section), "DESIGN.md 3.19 does not state %.4f" % recorded
