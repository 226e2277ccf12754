"""Worker for tests/test_qrows_gpu.py: one rank of a two-rank job, both ranks on cuda:0 (collectives over gloo). Each rank
quantizes its own half into a CHUNKED table — equal chunks (owner by multiply-high) and a custom partition (owner by search
over the rank offsets) —, then both gather ids that cross the boundary with the fused kernel, which reads the peer's rows
through its hipIpc mapping. The same on a DISTRIBUTED table, where the raw rows travel through the exchange."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist

import wholegraph_amd.torch as wgth
from wholegraph_amd.torch import quantized
from test_qrows_gpu import lookup_ids, narrowed, reference, same_bits


def scenario(comm, rank, mt, n_rows, dim, entries):
    x, raw, y = reference(n_rows, dim)                      # the same on every rank
    storage = wgth.create_wholememory_tensor(comm, mt, "cuda", [n_rows, wgth.quantized_row_bytes(dim)], torch.int8,
                                             [(wgth.quantized_row_bytes(dim) + 15) // 16 * 16, 1], entries)
    t = wgth.WholeMemoryQuantizedTensor(storage, dim)
    local, start = storage.get_local_tensor()
    mine = torch.arange(start, start + local.shape[0], dtype=torch.int64, device="cuda")
    t.scatter(torch.from_numpy(np.array(x[start:start + local.shape[0]])).cuda(), mine)   # each rank fills its own rows
    torch.cuda.synchronize()
    comm.barrier()
    assert np.array_equal(local.cpu().numpy().view(np.uint8), raw[start:start + local.shape[0]])
    ids_np = np.array(lookup_ids(n_rows, 1500 + rank))
    ids_np[10:14] = [n_rows // 2, n_rows // 2 - 1, start, max(start - 1, 0)]   # both sides of the boundary
    skip = ids_np < 0
    fused = mt == "chunked"
    for idt in (np.int64, np.int32):
        ids = torch.from_numpy(ids_np.astype(idt)).cuda()
        for dtype in ("float32", "bfloat16"):
            before = quantized.calls()
            got = t.gather(ids, force_dtype=getattr(torch, dtype))
            torch.cuda.synchronize()
            assert quantized.calls() == before + (1 if fused else 0)
            want = narrowed(y[np.maximum(ids_np, 0)], dtype)
            keep = torch.from_numpy(~skip)
            assert same_bits(got.cpu()[keep], want[keep]), (mt, dim, entries, dtype)
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
    for dim in (128, 11):
        scenario(comm, rank, "chunked", 4000, dim, None)             # equal chunks: same_chunk
        scenario(comm, rank, "chunked", 4001, dim, [1203, 2798])     # custom partition: the search over rank offsets
        scenario(comm, rank, "distributed", 4000, dim, None)
    comm.barrier()
    dist.barrier()
    print("RANK %d OK" % rank)
    wgth.finalize()


if __name__ == "__main__":
    main()
