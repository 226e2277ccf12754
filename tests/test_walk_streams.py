"""The random streams and steps of a random walk (include/wholememory/wholegraph_amd_ext.h section 2m) without a GPU: the
helpers the kernels use live in csrc/pcg.hpp, which compiles for the host. tests/cpp/walk_streams_test.cpp includes that
header alone, is built here with the host compiler's address and undefined-behaviour sanitizers (and -ffp-contract=off, as
the library is) and run as a process of its own; what it prints — mix, stream outputs, whole uniform and weighted walks of a
small CSR — is compared with tests/_walk_ref.py, the definition restated in Python over the oracle's generator, and with the
known answers the header states. Nothing is loaded into this interpreter but the oracle."""
import os
import subprocess

import numpy as np
import pytest

import _walk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX0 = 0xe220a8397b1dcdaf
STREAM0 = [2748719185, 1404529248, 2891244060, 1914411027]      # stream(42, 3, 0)
STREAM5 = [2746596618, 1305647937, 1544306493]                  # stream(42, 3, 5)
LENGTH, SEED = 5, 0xC0FFEE1234567


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk_streams") / "walk_streams_test")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "wholegraph_amd", "csrc"),
                         os.path.join(ROOT, "tests", "cpp", "walk_streams_test.cpp"), "-o", exe],
                        capture_output=True, timeout=300)
    assert cc.returncode == 0, cc.stderr.decode()[-4000:]
    return exe


def small_graph():
    """60 nodes of up to 9 neighbours, a hub of 300, a node without edges; a few col_ind entries outside the graph; weights
    with zeros, negatives, a NaN, runs of equal values and one node whose weights are all ineligible"""
    from test_graph_oracle import make_csr
    row_ptr, col = make_csr(60, 9, 7, heavy=[(3, 300), (4, 0), (5, 2)])
    col[::4] = 3                                     # the hub is visited
    col[[10, 57, 200]] = (-1, 60, (1 << 31) - 1)     # a damaged graph ends a walk
    rng = np.random.default_rng(11)
    weights = (rng.random(col.shape[0]) + 0.05).astype(np.float32)
    weights[rng.random(col.shape[0]) < 0.2] = 0.0
    weights[::9] = 0.5
    weights[row_ptr[5]:row_ptr[6]] = (0.0, -2.0)
    weights[row_ptr[3] + 17] = np.nan
    weights[row_ptr[3] + 18] = -0.0
    starts = np.concatenate([np.arange(12), [-1, 60, 3, 3, 3, 5, 4], rng.integers(0, 60, 21)]).astype(np.int64)
    return row_ptr, col, weights, starts


def run(program, tmp_path):
    row_ptr, col, weights, starts = small_graph()
    path = tmp_path / "graph.txt"
    numbers = [row_ptr.shape[0] - 1, col.shape[0], starts.shape[0], LENGTH, SEED]
    numbers += list(row_ptr) + list(col) + list(weights.view(np.uint32)) + list(starts)
    path.write_text(" ".join(str(int(x)) for x in numbers) + "\n")
    p = subprocess.run([program, str(path)], capture_output=True, timeout=300)
    assert p.returncode == 0, (p.stdout.decode()[-2000:], p.stderr.decode()[-4000:])
    return p.stdout.decode().splitlines()


def parse_walks(lines, tag, n):
    walks, eids = [], []
    for w, line in enumerate(l for l in lines if l.startswith(tag + " ")):
        head, _, rest = line.partition(":")
        assert int(head.split()[1]) == w
        nodes, _, edges = rest.partition("|")
        walks.append([int(x) for x in nodes.split()])
        eids.append([int(x) for x in edges.split()])
    assert len(walks) == n
    return np.array(walks, dtype=np.int64), np.array(eids, dtype=np.int64)


def test_known_answers_of_mix_and_stream(program, tmp_path):
    lines = run(program, tmp_path)
    assert lines[0] == "mix0 %016x" % MIX0
    assert [int(x) for x in lines[1].split()[1:]] == STREAM0 and lines[1].startswith("stream0")
    assert [int(x) for x in lines[2].split()[1:]] == STREAM5 and lines[2].startswith("stream5")
    # ... and the Python restatement gives the same
    assert ref.mix(0) == MIX0
    assert list(ref.stream(42, 3, 0, 4)) == STREAM0 and list(ref.stream(42, 3, 5, 3)) == STREAM5


def test_walks_of_the_header_equal_the_restated_definition(program, tmp_path):
    row_ptr, col, weights, starts = small_graph()
    lines = run(program, tmp_path)
    n = starts.shape[0]
    u_walks, u_eids = parse_walks(lines, "U", n)
    w_walks, w_eids = parse_walks(lines, "W", n)
    r_walks, r_eids = ref.uniform_walks(row_ptr, col, starts, LENGTH, SEED)
    assert np.array_equal(u_walks, r_walks) and np.array_equal(u_eids, r_eids)
    r_walks, r_eids = ref.weighted_walks(row_ptr, col, weights, starts, LENGTH, SEED)
    assert np.array_equal(w_walks, r_walks) and np.array_equal(w_eids, r_eids)
    # the graph exercises what it is meant to: refused starts, walks through the hub, walks ended by a node without edges, by a
    # node without an eligible neighbour and by a damaged col_ind entry, and steps onto ineligible weights never taken
    assert (u_walks[:, 0] < 0).sum() == 2 and (w_walks[:, 0] < 0).sum() == 2
    for walks, eids in ((u_walks, u_eids), (w_walks, w_eids)):
        assert ((walks[:, :-1] == 3) & (eids >= 0)).sum() >= 10, "steps from the hub"
        assert (eids < 0).any() and (eids[:, -1] >= 0).any()
        taken = eids[eids >= 0]
        assert np.array_equal(col[taken], walks[:, 1:][eids >= 0])
    assert (weights[w_eids[w_eids >= 0]] > 0).all()
    five = w_walks[:, 0] == 5
    assert five.any() and (w_walks[five, 1] == -1).all(), "node 5 has no eligible neighbour"
    damaged = {int(row_ptr.searchsorted(e, side="right") - 1) for e in (10, 57, 200)}
    ends = {int(row[row >= 0][-1]) for row, e in zip(u_walks, u_eids) if (row >= 0).any() and e[-1] < 0}
    assert ends & damaged or 4 in ends


def test_ladder_reference_holds_its_cases():
    """the lower bounds tests/test_walk_gpu.py relies on, on the reference walks of the ladder graph (no GPU needed to know
    that the ladder exercises its cases)"""
    u, w = ref.assert_ladder_measures()
    print("ladder measures: uniform %s, weighted %s" % (u, w))


def test_star_reference_statistics():
    """the distribution bounds of the GPU test are conditions on the definition itself: the device must equal the reference
    bit for bit, so they are checked here on the reference (uniform form; the weighted form of 8000 x 5 x 8 keys in plain
    Python loops is the GPU test's)"""
    row_ptr, col, _ = ref.star()
    starts = np.zeros(ref.STAR_WALKS, dtype=np.int64)
    walks, _ = ref.uniform_walks(row_ptr, col, starts, ref.STAR_LENGTH, ref.STAR_SEED)
    fit, independence = ref.star_statistics(walks, weighted=False)
    print("star, uniform: goodness of fit %.2f over 7 dof, independence %.2f over 49 dof" % (fit, independence))
    assert fit < 40.0 and independence < 110.0
