"""Worker for tests/test_gather_agg_gpu.py: one rank of a two-rank job over a CHUNKED table whose shards live in two
processes, so that the fused aggregation resolves rows of a peer's chunk (hipIpc mapping) — with equal chunks (owner by
multiply-high) and with a custom partition (owner by search over the rank offsets). Mode "devices": one GPU per rank, the
library's RCCL communicator; mode "shared": both ranks on cuda:0, collectives over gloo."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist

import wholegraph_amd.torch as wgth
from wholegraph_amd.torch import gather_aggregation
from wholegraph_amd.torch.aggregation import agg_concat
from test_gather_agg_gpu import block, ref_forward, table_values


def scenario(comm, rank, world, dtype, n_rows, dim, entries):
    emb = wgth.create_embedding(comm, "chunked", "cuda", dtype, [n_rows, dim], embedding_entry_partition=entries)
    full = table_values(np.random.default_rng(100 + dim), n_rows, dim, dtype)   # the same on every rank
    local, start = emb.get_embedding_tensor().get_local_tensor()
    local.copy_(full[start:start + local.shape[0]].cuda())
    torch.cuda.synchronize()
    comm.barrier()
    rng = np.random.default_rng(7 + rank)
    n_dst, n_src = 211, 900
    row_ptr, col = block(rng, n_dst, n_src, 40)
    ids_np = rng.integers(0, n_rows, n_src)
    ids_np[:4] = [0, n_rows - 1, n_rows // 2, n_rows // 2 - 1]   # first and last row of both chunks' neighbourhood
    rp, ci = torch.from_numpy(row_ptr).cuda(), torch.from_numpy(col).cuda()
    x_np = full.float().numpy()[ids_np]
    for idt in (np.int64, np.int32):
        ids = torch.from_numpy(ids_np.astype(idt)).cuda()
        for aggr in ("mean", "sum"):
            before = gather_aggregation.calls()
            got = wgth.gather_agg_concat(emb, ids, rp, ci, aggr)
            assert gather_aggregation.calls() == before + 1
            two = agg_concat(emb.gather(ids, force_dtype=torch.float32), rp, ci, aggr)
            torch.cuda.synchronize()
            assert torch.equal(got, two), (dtype, dim, entries, aggr)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), ref_forward(row_ptr, col, x_np, aggr).view(np.uint32))
    comm.barrier()
    wgth.destroy_embedding(emb)


def main():
    rank, world, port, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    if mode == "devices":
        assert torch.cuda.device_count() >= world
        torch.cuda.set_device(rank)
    else:
        torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl" if mode == "devices" else "gloo", init_method="env://", rank=rank,
                            world_size=world)
    wgth.init(rank, world, rank, world, "warn")
    comm = wgth.get_global_communicator()
    assert comm.get_size() == world
    for dtype, dim in ((torch.float32, 128), (torch.bfloat16, 128), (torch.float16, 11), (torch.float32, 33)):
        scenario(comm, rank, world, dtype, 4000, dim, None)           # equal chunks: same_chunk
        scenario(comm, rank, world, dtype, 4001, dim, [1203, 2798])   # custom partition: the search over rank offsets
    comm.barrier()
    dist.barrier()
    print("RANK %d OK" % rank)
    wgth.finalize()


if __name__ == "__main__":
    main()
