"""Worker for tests/test_qagg_gpu.py: one rank of a two-rank job, both ranks on cuda:0 (collectives over gloo). Each rank
quantizes its own half into a CHUNKED table — equal chunks (owner by multiply-high) and a custom partition (owner by search
over the rank offsets) —, then both run the fused aggregation over node ids that land on both ranks and on the first and
the last row of each: the peer's rows are read through its hipIpc mapping. Compared, bit for bit, with the composition
agg_concat(table.gather(ids))."""
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
from test_qagg_gpu import N_SRC, ladder_block, node_ids, same_bits
from test_qrows_gpu import reference


def scenario(comm, rank, n_rows, dim, row_align, entries):
    x, raw, y = reference(n_rows, dim)                      # the same on every rank
    rb = wgth.quantized_row_bytes(dim)
    storage = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [n_rows, rb], torch.int8,
                                             [(rb + row_align - 1) // row_align * row_align, 1], entries)
    t = wgth.WholeMemoryQuantizedTensor(storage, dim)
    local, start = storage.get_local_tensor()
    mine = torch.arange(start, start + local.shape[0], dtype=torch.int64, device="cuda")
    t.scatter(torch.from_numpy(np.array(x[start:start + local.shape[0]])).cuda(), mine)   # each rank fills its own rows
    torch.cuda.synchronize()
    comm.barrier()
    bound = local.shape[0] if rank == 0 else start          # rank 1's first row
    assert 0 < bound < n_rows and (entries is None or bound == entries[0]), (bound, entries)
    ids_np = np.array(node_ids(n_rows))
    ids_np[4:8] = [bound - 1, bound, n_rows - 1, 0]         # the last and the first row of each rank, among the targets ...
    ids_np[N_SRC // 2:N_SRC // 2 + 4] = [bound, bound - 1, 0, n_rows - 1]   # ... and among the neighbours only
    assert (ids_np < bound).sum() > 50 and (ids_np >= bound).sum() > 50
    row_ptr, col = ladder_block()
    rp, ci = torch.from_numpy(np.array(row_ptr)).cuda(), torch.from_numpy(np.array(col)).cuda()
    assert gather_aggregation.takes_fused_route(t)
    for idt in (np.int64, np.int32):
        ids = torch.from_numpy(ids_np.astype(idt)).cuda()
        for aggr in ("sum", "mean"):
            before = gather_aggregation.quantized_calls()
            got = wgth.gather_agg_concat(t, ids, rp, ci, aggr)
            torch.cuda.synchronize()
            assert gather_aggregation.quantized_calls() == before + 1
            assert same_bits(got, agg_concat(t.gather(ids), rp, ci, aggr)), (dim, row_align, entries, aggr, idt)
            # the self half is the dequantized rows themselves (the numpy restatement of tests/test_qrows_surface.py)
            assert same_bits(got[:, dim:].contiguous(), torch.from_numpy(np.array(y[ids_np[:got.shape[0]]])))
    comm.barrier()
    wgth.destroy_wholememory_tensor(storage)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group(backend="gloo", init_method="env://", rank=rank, world_size=world)
    wgth.init(rank, world, rank, world, "warn")
    comm = wgth.get_global_communicator()
    assert comm.get_size() == world
    for dim, row_align in ((128, 4), (128, 16), (7, 4)):
        scenario(comm, rank, 4000, dim, row_align, None)             # equal chunks: same_chunk
        scenario(comm, rank, 4001, dim, row_align, [1203, 2798])     # custom partition: the search over rank offsets
    comm.barrier()
    dist.barrier()
    print("RANK %d OK" % rank)
    wgth.finalize()


if __name__ == "__main__":
    main()
