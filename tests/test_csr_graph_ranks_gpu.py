"""Every op that reads the WholeMemory CSR graph, on a graph that lives on 2 and on 3 ranks (MI355X; all ranks share cuda:0).

On one rank a CHUNKED tensor is a single chunk: gref_load (csrc/kernels/gref_view.cuh) finds owner 0 and subtracts a start of
0 whatever it computes. Here the ladder graph of tests/test_sampler_edges_gpu.py is split over the ranks in every layout the
ops read — equal chunks (owner by division), custom entry partitions (owner by search; csr_row_ptr cut between s and e of a
batch node, the edge arrays cut inside the hub's row and inside a short batch row, an empty or one-entry middle rank), the same
chunks behind odd storage offsets, CONTINUOUS, host-located CHUNKED and DISTRIBUTED — and every rank asks for a batch of its
own. What can only go wrong there: an owner taken from the element index instead of the byte offset, a chunk start that is not
subtracted, a storage offset added after the owner was resolved, a row or a neighbour list that straddles a cut. The checks
and references are those of the single-rank tests (tests/_csr_graph_checks.py), fed the full arrays, all exact; the worker
(tests/_csr_ranks_worker.py) states the layouts and what each rank passes.

A launch is one op family on one world size: the worker runs every layout and prints a line per layout. Launches are shared
by the tests that read them."""
import os
import subprocess
import sys
import tempfile
import time

import pytest

import _csr_graph_checks as checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (2, 3)
GROUPS = ("samplers", "hops", "walks", "neg_isub")
LAYOUTS = ("chunked", "custom-hub", "custom-short", "views", "continuous", "host", "distributed")
TIMEOUT = 120          # seconds: a safety net, a launch takes a fraction of it
_LAUNCHES = {}


def launch(world, group):
    """-> [(return code, output) per rank] of one worker job, run once. A rank that fails ends the others: they would wait
    for it in a collective until the timeout."""
    if (world, group) not in _LAUNCHES:
        from test_distributed_cpu import free_port
        port = str(free_port())
        env = dict(os.environ, OMP_NUM_THREADS="1")
        logs = [tempfile.TemporaryFile() for _ in range(world)]
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_csr_ranks_worker.py"), str(r), str(world), port, group],
                                  env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
        deadline = time.monotonic() + TIMEOUT
        try:
            while any(p.poll() is None for p in procs):
                if time.monotonic() > deadline or any(p.returncode not in (None, 0) for p in procs):
                    break
                try:
                    next(p for p in procs if p.returncode is None).wait(timeout=0.2)
                except subprocess.TimeoutExpired:
                    pass
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                p.wait()
        outs = []
        for log in logs:
            log.seek(0)
            outs.append(log.read().decode(errors="replace"))
            log.close()
        _LAUNCHES[(world, group)] = [(p.returncode, o) for p, o in zip(procs, outs)]
    return _LAUNCHES[(world, group)]


def tails(ranks):
    return "\n=====\n".join(o[-2500:] for _, o in ranks)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("world", WORLDS)
def test_graph_ops_on_a_graph_split_over_ranks(wm_lib, world, group):
    ranks = launch(world, group)
    print("\n".join(line for line in ranks[0][1].splitlines() if line.startswith(("CUTS", "EMPTY")) or "taken" in line))
    for r, (code, out) in enumerate(ranks):
        assert code == 0 and ("RANK %d OK" % r) in out, "rank %d failed:\n%s" % (r, tails(ranks))
        for layout in LAYOUTS:
            assert ("RANK %d %s OK" % (r, layout)) in out, "rank %d did not finish %s:\n%s" % (r, layout, tails(ranks))


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_weighted_sampler_on_a_distributed_graph_equals_the_oracle(wm_lib, world):
    """The weighted one-hop sampler on a DISTRIBUTED graph against oracle.sample_weighted, on every rank (the `samplers`
    launch reports it on a line of its own). The C entry point has no route for DISTRIBUTED tensors; the Python op composes
    one (wholegraph_ops._weighted_sample_via_gather), a collective."""
    ranks = launch(world, "samplers")
    for r, (code, out) in enumerate(ranks):
        assert ("RANK %d distributed weighted sampler OK" % r) in out, "rank %d:\n%s" % (r, tails(ranks))


@pytest.mark.parametrize("world", WORLDS)
def test_the_cuts_fall_where_the_cases_say(world):
    """the partition arrays alone (no GPU): a later change of the ladder's generator cannot silently move a cut to a row
    boundary. assert_custom_partitions is what the worker runs before it creates a tensor."""
    from test_sampler_edges_gpu import ladder_graph
    row_ptr = ladder_graph()[0]
    n_nodes, n_edges = row_ptr.shape[0] - 1, int(row_ptr[-1])
    batch = [int(v) for v in checks.batch()]
    for middle in ((0,) if world == 2 else (0, 1)):      # an empty middle rank, and the one entry a refusal leaves it
        for cut in ("hub", "short"):
            p = checks.assert_custom_partitions(world, cut, middle)
            row, edge, v, x = p["row"], p["edge"], p["row_node"], p["edge_node"]
            print("world %d, cut %s, middle %d: csr_row_ptr %s after node %d, edge arrays %s in the row of node %d [%d, %d)" % (
                world, cut, middle, row, v, edge, x, row_ptr[x], row_ptr[x + 1]))
            # the same statements, written out on the arrays
            assert sum(row) == n_nodes + 1 and sum(edge) == n_edges
            assert len(set(row)) > 1 and len(set(edge)) > 1
            assert v in batch and row[0] == v + 1                      # row_ptr[v] ends rank 0, row_ptr[v + 1] starts the next
            s, e = int(row_ptr[x]), int(row_ptr[x + 1])
            assert s < edge[0] and edge[0] + (edge[1] if world == 3 else 0) < e
            assert (e - s == checks.HUB_DEGREE) if cut == "hub" else (x in batch and 2 <= e - s <= 32)
            if world == 3:
                assert row[1] == edge[1] == middle
            if world == 2:      # two ranks divide unless the first partition is the smaller one
                assert row[0] < row[1] and edge[0] < edge[1]
