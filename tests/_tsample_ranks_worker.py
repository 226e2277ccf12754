"""Worker for tests/test_tsample_ranks_gpu.py: one rank of a job of 2 ranks, both on cuda:0 (collectives over gloo), which runs
the temporal sampler on the temporal ladder (tests/_tsample_ref.py) split over the ranks. argv: rank, world, port.

Every rank builds the same full arrays on the host and fills its own part of each tensor (tests/_csr_graph_checks.wm_array,
imported unchanged); the reference is the single-rank one, fed the full arrays. Each rank passes a batch of its own: the
ladder's centres and their times rotated by 17 * rank, int32 ids on rank 1 and int64 ids on rank 0. The layouts, and what the
worker asserts about each before its first GPU call:
  chunked      CHUNKED device, equal partition: the owner by division
  custom       CHUNKED device, entry partitions: csr_row_ptr cut between s and e of node 7 (the hub: s is read from rank 0, e
               from rank 1), col_ind and the edge TIMES cut strictly inside the hub's row; the first partition is the smaller
               one, so the owner is found by search
  distributed  DISTRIBUTED device: the C entry point has no route, wholegraph_ops composes one (a collective)
A rank prints `RANK r <layout> OK` per layout and `RANK r OK` at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import _tsample_ref as ref
from _csr_graph_checks import owner_of, searches, wm_array

LAYOUTS = ("chunked", "custom", "distributed")
HUB = 7
CASES = (("uniform", ref.LADDER_M, True, None), ("last", 5, False, 50), ("uniform", -1, True, 50))


def rank_batch(rank):
    """-> (centres, centre times) as this rank passes them"""
    _, _, _, starts, ctimes = ref.temporal_ladder()
    return np.roll(starts, -17 * rank).astype(np.int32 if rank == 1 else np.int64), np.roll(ctimes, -17 * rank)


def custom_partitions(world):
    """-> {"row": of csr_row_ptr, "edge": of col_ind and the edge times}, with the assertions the docstring above makes"""
    row_ptr = ref.temporal_ladder()[0]
    n_nodes, n_edges = row_ptr.shape[0] - 1, int(row_ptr[-1])
    s, e = int(row_ptr[HUB]), int(row_ptr[HUB + 1])
    assert world == 2 and e - s == 5000
    row, edge = [HUB + 1, n_nodes + 1 - (HUB + 1)], [s + 2500, n_edges - (s + 2500)]
    assert owner_of(row, HUB) == 0 and owner_of(row, HUB + 1) == 1
    assert s < edge[0] < e and owner_of(edge, s) == 0 and owner_of(edge, e - 1) == 1
    assert searches(row) and searches(edge) and sum(row) == n_nodes + 1 and sum(edge) == n_edges
    return {"row": row, "edge": edge}


def main():
    import torch
    import torch.distributed as dist
    import wholegraph_amd.torch as wgth
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", init_method="env://", rank=rank, world_size=world)
    wgth.init(rank, world, rank, world, "warn")
    comm = wgth.get_global_communicator()
    assert comm.get_size() == world
    row_ptr, col, etime, _, _ = ref.temporal_ladder()
    centres, times = rank_batch(rank)
    assert HUB in centres.tolist()
    wants = [ref.temporal_sample(row_ptr, col, etime, centres, times, m, strategy, inclusive, window, ref.LADDER_SEED + rank,
                                 draw=ref.cached_draws) for strategy, m, inclusive, window in CASES]
    dev, dev_t = torch.from_numpy(centres).cuda(), torch.from_numpy(times).cuda()
    for k, layout in enumerate(LAYOUTS):
        col_dtype = (np.int32, np.int64)[k % 2]
        parts = custom_partitions(world) if layout == "custom" else {"row": None, "edge": None}
        mt = "chunked" if layout == "custom" else layout
        ts = [wm_array(comm, mt, np.array(row_ptr), "cuda", parts["row"]), wm_array(comm, mt, col.astype(col_dtype), "cuda", parts["edge"]),
              wm_array(comm, mt, np.array(etime), "cuda", parts["edge"])]
        comm.barrier()      # every rank has filled its part
        g = wgth.GraphStructure()
        g.set_csr_graph(ts[0], ts[1])
        g.set_edge_attribute("t", ts[2])
        for (strategy, m, inclusive, window), want in zip(CASES, wants):
            got = g.temporal_sample_one_hop("t", dev, dev_t, m, strategy=strategy, inclusive=inclusive, time_window=window,
                                            random_seed=ref.LADDER_SEED + rank, need_center_local_output=True, need_edge_output=True)
            what = "rank %d, %s, %s, M = %d" % (rank, layout, strategy, m)
            assert len(got) == 4 and got[1].dtype == torch.from_numpy(np.empty(0, dtype=col_dtype)).dtype, what
            for name, a, b in zip(("offsets", "ids", "center local ids", "edge ids"), got, want):
                assert np.array_equal(a.cpu().numpy().astype(np.int64), np.asarray(b).astype(np.int64)), "%s differ: %s" % (name, what)
        torch.cuda.synchronize()
        comm.barrier()      # nobody frees its part while a peer still reads it
        for t in ts:
            wgth.destroy_wholememory_tensor(t)
        print("RANK %d %s OK (col %s)" % (rank, layout, np.dtype(col_dtype).name), flush=True)
    comm.barrier()
    dist.barrier()
    print("RANK %d OK" % rank, flush=True)
    wgth.finalize()


if __name__ == "__main__":
    main()
