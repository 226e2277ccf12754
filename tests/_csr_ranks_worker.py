"""Worker for tests/test_csr_graph_ranks_gpu.py: one rank of a job of 2 or 3 ranks, all of them on cuda:0 (collectives over
gloo), which runs one group of the ops that read the WholeMemory CSR graph on a graph split over the ranks. argv: rank, world,
port, group (samplers | hops | walks | neg_isub).

Every rank builds the same full arrays on the host (tests/_csr_graph_checks.py) and fills its own part of each tensor; the
checks and their references are those of the single-rank tests, fed the full arrays. Each rank passes a batch of its own: the
ladder's centres or batch() rotated by 17 * rank, seeds moved by the rank's number, int32 ids on rank 1 and int64 ids elsewhere
(the fused hop and the chain take ids of the column dtype only), and the last rank passes an empty batch. The layouts, and what
the worker asserts about each before its first GPU call:
  chunked       CHUNKED device, equal partition: the owner by division; the last chunk of the edge arrays is the shortest
  custom-hub    CHUNKED device, the entry partitions of custom_partitions(world, "hub"): the owner by search; csr_row_ptr cut
  custom-short  between s and e of a batch node, the edge arrays cut inside the hub's row / a short batch row; three ranks: the
                middle rank holds nothing, or one entry where the library refuses an empty partition
  views         CHUNKED device, equal partition, every array a sub-tensor view at an odd storage offset into a poisoned array
  continuous    CONTINUOUS device, equal partition
  host          CHUNKED host, equal partition, the subset fan-outs
  distributed   DISTRIBUTED device, the subset fan-outs: the samplers are collectives and equal the oracle, the fused hop and
                the chain decline or equal the two ops, the other ops answer NOT_IMPLEMENTED
A rank prints `RANK r <layout> OK` per layout and `RANK r OK` at the end. The weighted sampler on the DISTRIBUTED graph is
reported on a line of its own, `RANK r distributed weighted sampler OK` or `... FAILED: <why>`, and does not stop the rank."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiprocessing

import numpy as np

import _csr_graph_checks as checks
from test_sampler_edges_gpu import UNWEIGHTED_SUBSET, WEIGHTED_SUBSET, ladder_graph

GROUPS = ("samplers", "hops", "walks", "neg_isub")
LAYOUTS = ("chunked", "custom-hub", "custom-short", "views", "continuous", "host", "distributed")


def rank_batches(rank, world):
    """-> (the ladder's centres, batch()) as this rank passes them"""
    id_dtype = np.int32 if rank == 1 else np.int64
    keep = slice(0, 0) if rank == world - 1 else slice(None)      # the last rank asks for nothing
    return (np.roll(ladder_graph()[2], -17 * rank).astype(id_dtype)[keep],
            np.roll(checks.batch(), -17 * rank).astype(id_dtype)[keep])


def start_slow_references(group, rank, nodes):
    """The Python references of the weighted and the node2vec walks take a second or two each. Children forked HERE — before
    torch is imported, so that they hold no GPU and no thread — compute them while this process starts up.
    -> (pool, pending results) or None"""
    jobs = {"walks": [(checks.walk_references, nodes, rank), (checks.node2vec_reference, False, nodes, rank),
                      (checks.node2vec_reference, True, nodes, rank)],
            "neg_isub": [(checks.walk_references, nodes, rank)]}.get(group, [])
    if not jobs or nodes.shape[0] == 0:
        return None
    checks.graph(False), checks.graph(True)      # (built once, inherited by the children)
    pool = multiprocessing.get_context("fork").Pool(len(jobs))
    return pool, [pool.apply_async(checks.references_made_by, job) for job in jobs]


def adopt_slow_references(started):
    if started is not None:
        pool, pending = started
        for result in pending:
            checks.adopt_references(result.get())
        pool.close()
        pool.join()


if __name__ == "__main__":
    SLOW_REFERENCES = start_slow_references(sys.argv[4], int(sys.argv[1]), rank_batches(int(sys.argv[1]), int(sys.argv[2]))[1])

import torch
import torch.distributed as dist

import wholegraph_amd.torch as wgth
from wholegraph_amd import binding


def entries_of(t, world):
    """the entries every rank holds of a 1-D tensor, from the byte sizes the library planned"""
    sizes = (C.c_size_t * world)()
    binding.check(binding.lib().wholememory_get_rank_partition_sizes(sizes, t._handle()))
    element = torch.tensor([], dtype=t.dtype).element_size()
    assert all(s % element == 0 for s in sizes)
    return [int(s) // element for s in sizes]


def middle_entries(comm, world):
    """what the middle of three ranks holds in the custom partitions: nothing if the library takes an empty partition, else
    one entry (the refusal is INVALID_VALUE, answered on every rank before anything is allocated)"""
    if world < 3:
        return 0
    part = checks.custom_partitions(world, "hub", 0)["row"]
    try:
        t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [sum(part)], torch.int64, [1], part)
    except binding.WholeMemoryError as e:
        assert e.code == 7, e      # WHOLEMEMORY_INVALID_VALUE
        return 1
    wgth.destroy_wholememory_tensor(t)
    return 0


def build(comm, rank, world, layout, col_dtype, in_order, middle):
    """the graph in one layout, with the layout's own assertions -> checks.Graph"""
    if layout in ("custom-hub", "custom-short"):
        p = checks.assert_custom_partitions(world, layout[len("custom-"):], middle)
        h = checks.Graph(comm, "chunked", col_dtype, in_order, entries=p)
        for t, part in zip(h.tensors, ("row", "edge", "edge", "edge")):
            got = entries_of(t, world)
            assert got == p[part] and checks.searches(got), (layout, part, got, p[part])
        if rank == 0 and not in_order:
            print("CUTS %s world %d: csr_row_ptr %s after node %d, edge arrays %s in the row of node %d" % (
                layout, world, p["row"], p["row_node"], p["edge"], p["edge_node"]), flush=True)
    elif layout == "views":
        h = checks.Views(comm, "chunked", col_dtype, in_order)
        assert all(t.storage_offset() == lead for t, lead in zip(h.tensors, (checks.ROW_AT, checks.COL_AT, checks.WEIGHT_AT,
                                                                                checks.ATTR_AT)))
    elif layout == "host":
        h = checks.Graph(comm, "chunked", col_dtype, in_order, loc="cpu")
    else:
        h = checks.Graph(comm, layout, col_dtype, in_order)
    if layout == "chunked":      # equal chunks: ceil(n / world) entries each, the last chunk of the edge arrays shorter
        for k, t in enumerate(h.tensors):
            n = t.shape[0]
            per_rank = (n + world - 1) // world
            starts = t.get_all_chunked_tensor()[1]
            assert starts == [min(r * per_rank, n) for r in range(world)], (starts, n)
            got = entries_of(t, world)
            assert not checks.searches(got) and (k == 0 or 0 < got[-1] < got[0]), got
    comm.barrier()      # every rank has filled its part
    return h


def run_layout(comm, rank, world, group, layout, col_dtype, middle, centers, nodes):
    """-> (what to print about the layout, or "", the failure of the weighted sampler on DISTRIBUTED or None)"""
    distributed = layout == "distributed"
    note, weighted_failure = "", None
    h = build(comm, rank, world, layout, col_dtype, False, middle)
    if group == "samplers":
        subset = layout in ("host", "distributed")
        unweighted = UNWEIGHTED_SUBSET if subset else checks.UNWEIGHTED_FANOUTS
        weighted = WEIGHTED_SUBSET if subset else checks.WEIGHTED_FANOUTS
        checks.check_samplers(h, col_dtype, centers, rank, unweighted, () if distributed else weighted)
        if distributed:
            try:
                checks.check_samplers(h, col_dtype, centers, rank, (), weighted)
            except Exception as e:      # (reported on a line of its own: the other checks of the launch still count)
                weighted_failure = "%s: %s" % (type(e).__name__, e)
    elif group == "hops":
        hops = checks.check_fused_hop(h, col_dtype, centers, rank, may_decline=distributed)
        chains = checks.check_chain(h, col_dtype, centers[:101], rank, may_decline=distributed)
        if distributed:
            note = "fused hop taken %d times, chain taken %d times" % (hops, chains)
        else:
            checks.check_deferred_chain(comm, h, col_dtype, centers[:101], rank)
    elif distributed:
        checks.check_not_implemented(h, nodes, ("random_walk", "node2vec_walk") if group == "walks"
                                     else ("negative_sample", "induced_subgraph"))
    else:
        ordered = build(comm, rank, world, layout, col_dtype, True, middle)
        if group == "walks":
            checks.check_walks(h, col_dtype, nodes, rank)
            checks.check_node2vec(h, col_dtype, nodes, rank)
            checks.check_node2vec(ordered, col_dtype, nodes, rank)
        else:
            checks.check_negatives(h, col_dtype, nodes, rank)
            checks.check_negatives(ordered, col_dtype, nodes, rank)
            with_hub = np.concatenate([nodes, np.array([checks.hub_node()], dtype=nodes.dtype)]) if nodes.shape[0] else nodes
            checks.check_induced_subgraph(h, col_dtype, with_hub)
            checks.check_saint(h, col_dtype, nodes, rank)
        torch.cuda.synchronize()
        comm.barrier()      # nobody frees its part while a peer still reads it
        ordered.destroy()
    torch.cuda.synchronize()
    comm.barrier()
    h.destroy()
    return note, weighted_failure


def main():
    rank, world, port, group = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    assert group in GROUPS
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", init_method="env://", rank=rank, world_size=world)
    wgth.init(rank, world, rank, world, "warn")
    comm = wgth.get_global_communicator()
    assert comm.get_size() == world
    centers, nodes = rank_batches(rank, world)
    middle = middle_entries(comm, world)
    adopt_slow_references(SLOW_REFERENCES)
    if rank == 0 and world == 3:
        print("EMPTY MIDDLE PARTITION %s" % ("refused (INVALID_VALUE): the middle rank holds one entry" if middle else "accepted"),
              flush=True)
    for k, layout in enumerate(LAYOUTS):
        col_dtype = (np.int32, np.int64)[(k + world) % 2]      # both dtypes on every layout, over the two world sizes
        note, weighted_failure = run_layout(comm, rank, world, group, layout, col_dtype, middle, centers, nodes)
        print("RANK %d %s OK (col %s)%s" % (rank, layout, np.dtype(col_dtype).name, ": " + note if note else ""), flush=True)
        if group == "samplers" and layout == "distributed":
            print("RANK %d distributed weighted sampler %s" % (rank, "OK" if weighted_failure is None
                                                               else "FAILED: " + weighted_failure), flush=True)
    comm.barrier()
    dist.barrier()
    print("RANK %d OK" % rank, flush=True)
    wgth.finalize()


if __name__ == "__main__":
    main()
