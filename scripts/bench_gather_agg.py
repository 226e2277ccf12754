#!/usr/bin/env python3
"""Timing of `gather_agg_concat` — agg_concat straight from a WholeMemory table (wholegraph_amd/torch/gather_aggregation.py
-> csrc/kernels/agg_gather.hip) — against the two ops it replaces, on one MI355X; prints ONE JSON line.

Shapes (those of scripts/bench_sage_agg.py), over ONE table per dtype:
  a  uniform: n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M node ids drawn uniformly from the table
  c  layer 0 (the outermost block) of a BASELINE config 5 sample: 1024 seeds, fan-outs 30,30, on a graph built the way
     bench.py --op sample_gather builds it, with as many nodes as the table has rows; the node ids are the sampler's
The table is CHUNKED on the device, --table-rows x --dim (default 100 M x 128: the C2 table); when that does not fit in
70 % of the free device memory the rows are halved until it does, and the size used is reported.

Per shape and table dtype (float32, then bfloat16), in one process on one block, median of --reps calls after --warmup:
  fused     gather_agg_concat(emb, ids, ...)
  two_op    agg_concat(emb.gather(ids, force_dtype=float32), ...), and its parts: the gather alone, the fp32 agg_concat alone
The results are checked to be equal bit for bit first. Gate (reported, not asserted): the fused forward takes no longer
than the two-op median times the two-op's own max / median spread over its timed calls.
Algorithmic bytes, T = bytes of a table element, I = bytes of a node id:
  two ops  n_src (I + T F + 4 F) + E (4 + 4 F) + n_dst (4 + 12 F)
  fused    E (4 + I + T F) + n_dst (4 + I + T F + 8 F)
The fraction is of 8 TB/s, on the fused byte count."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PEAK = 8.0e12


def c5_layer0(wgth, comm, nodes, avg, seeds_n, fanouts):
    """layer 0 of one sample on the bench.py sample_gather graph (CHUNKED, one GPU): row_ptr, col_ind and the node ids"""
    import torch
    from bench_sage_agg import powerlaw_ids
    gen = torch.Generator(device="cuda").manual_seed(1)
    row = torch.zeros(nodes + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.randint(0, 2 * avg + 1, (nodes,), device="cuda", generator=gen), 0, out=row[1:])
    edges = int(row[-1])
    wrow = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [nodes + 1], torch.int64, [1])
    wcol = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [edges], torch.int32, [1])
    wrow.get_local_tensor()[0].copy_(row)
    del row
    lcol = wcol.get_local_tensor()[0]
    gen2 = torch.Generator(device="cuda").manual_seed(100)
    for s0 in range(0, edges, 1 << 28):
        e0 = min(edges, s0 + (1 << 28))
        lcol[s0:e0] = powerlaw_ids(nodes, e0 - s0, 0.8, gen2)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    seeds = torch.randint(0, nodes, (seeds_n,), device="cuda", generator=gen2, dtype=torch.int32)
    tg, _, rp, ci = g.multilayer_sample_without_replacement(seeds, fanouts, random_seeds=[11, 12])
    out = rp[0].clone(), ci[0].clone(), tg[0].clone()
    del g, lcol
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
    torch.cuda.synchronize()
    return out


def make_table(wgth, comm, rows, dim, dtype):
    import torch
    emb = wgth.create_embedding(comm, "chunked", "cuda", dtype, [rows, dim])
    local = emb.get_embedding_tensor().get_local_tensor()[0]
    gen = torch.Generator(device="cuda").manual_seed(5)
    step = max(1, (1 << 28) // dim)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        local[r0:r1] = torch.randn((r1 - r0, dim), device="cuda", generator=gen).to(dtype)
    torch.cuda.synchronize()
    return emb


def run_shape(name, emb, ids, row_ptr, col_ind, dim, dtype, warmup, reps):
    import torch
    import wholegraph_amd.torch as wgth
    from bench_sage_agg import timed_all
    from wholegraph_amd.torch import gather_aggregation
    from wholegraph_amd.torch.aggregation import agg_concat
    n_dst, E, n_src = row_ptr.numel() - 1, col_ind.numel(), ids.numel()

    def fused():
        return wgth.gather_agg_concat(emb, ids, row_ptr, col_ind, "mean")

    def gather():
        return emb.gather(ids, force_dtype=torch.float32)

    def two_op():
        return agg_concat(gather(), row_ptr, col_ind, "mean")
    before = gather_aggregation.calls()
    a, b = fused(), two_op()
    assert gather_aggregation.calls() == before + 1, "the fused kernel did not run"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "fused and two-op results differ"
    del a, b
    x = gather()

    def stats(ms):
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    f = stats(timed_all(fused, warmup, reps))
    t = stats(timed_all(two_op, warmup, reps))
    gt = stats(timed_all(gather, warmup, reps))
    ag = stats(timed_all(lambda: agg_concat(x, row_ptr, col_ind, "mean"), warmup, reps))
    f2 = stats(timed_all(fused, warmup, reps))   # (a second pass behind the others: the order of the runs is not the result)
    T, I = emb.get_embedding_tensor().dtype.itemsize, ids.element_size()
    two_bytes = n_src * (I + T * dim + 4 * dim) + E * (4 + 4 * dim) + n_dst * (4 + 12 * dim)
    fused_bytes = E * (4 + I + T * dim) + n_dst * (4 + I + T * dim + 8 * dim)
    allowance = t["median_ms"] * (t["max_ms"] / t["median_ms"])
    res = {"shape": name, "table_dtype": str(dtype).replace("torch.", ""), "id_dtype": str(ids.dtype).replace("torch.", ""),
           "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": dim,
           "fused": f, "fused_second_pass": f2, "two_op": t, "two_op_gather": gt, "two_op_agg_concat": ag,
           "fused_bytes": fused_bytes, "two_op_bytes": two_bytes, "bytes_ratio": round(fused_bytes / two_bytes, 3),
           "fused_GBps": round(fused_bytes / f["median_ms"] / 1e6, 1),
           "fused_frac_8TBps": round(fused_bytes / f["median_ms"] / 1e-3 / PEAK, 4),
           "two_op_GBps": round(two_bytes / t["median_ms"] / 1e6, 1),
           "fused_over_two_op": round(f["median_ms"] / t["median_ms"], 3),
           "two_op_spread_max_over_median": round(t["max_ms"] / t["median_ms"], 3),
           "gate_fused_within_two_op_spread": bool(f["median_ms"] <= allowance)}
    del x
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--table-rows", type=int, default=100_000_000)
    p.add_argument("--n-dst", type=int, default=333_334)
    p.add_argument("--fanout", type=int, default=30)
    p.add_argument("--n-src", type=int, default=2_000_000)
    p.add_argument("--shapes", default="a,c")
    p.add_argument("--dtypes", default="float32,bfloat16")
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_gather_agg.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)

    rows = a.table_rows
    free, _ = torch.cuda.mem_get_info()
    while rows * a.dim * 4 > 0.7 * free and rows > 1_000_000:
        rows //= 2
    blocks = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    for shape in a.shapes.split(","):
        if shape == "a":
            row_ptr = torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout
            col = torch.randint(0, a.n_src, (a.n_dst * a.fanout,), device="cuda", generator=gen, dtype=torch.int32)
            ids = torch.randint(0, rows, (a.n_src,), device="cuda", generator=gen, dtype=torch.int64)
            blocks.append(("a_uniform", ids, row_ptr, col))
        elif shape == "c":
            rp, ci, gids = c5_layer0(wgth, comm, rows, 29, 1024, [30, 30])
            blocks.append(("c_c5_layer0", gids, rp, ci))
    results = []
    for dt in a.dtypes.split(","):
        dtype = getattr(torch, dt)
        emb = make_table(wgth, comm, rows, a.dim, dtype)
        for name, ids, rp, ci in blocks:
            results.append(run_shape(name, emb, ids, rp, ci, a.dim, dtype, a.warmup, a.reps))
        wgth.destroy_embedding(emb)
        torch.cuda.empty_cache()
    line = {"bench": "gather_agg", "peak_Bps": PEAK, "table_rows": rows, "table_rows_asked": a.table_rows, "dim": a.dim,
            "table_GB_fp32": round(rows * a.dim * 4 / 1e9, 2), "warmup": a.warmup, "reps": a.reps, "results": results,
            "gate_all": bool(all(r["gate_fused_within_two_op_spread"] for r in results))}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
