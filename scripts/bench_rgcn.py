#!/usr/bin/env python3
"""Timing of the relation-typed aggregation (wholegraph_amd/torch/rel_aggregation.py -> csrc/kernels/agg_rel.hip) on one
MI355X; prints ONE JSON line.

Shape: a sampled block, n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M, F = 128, "mean", edge types uniform in
[0, R) for each R of `--relations`.

Per R, the median of `--reps` calls after `--warmup`: the forward and the backward of agg_concat_rel, and in the same
process on the same block the route a user had before this op: R calls of agg_concat on the per-relation sub-blocks plus
the concat of their first F columns and the self rows (its backward through autograd). The sub-blocks are built once,
outside the timed region — a user would pay for the R masks and prefix sums in every batch too. The fused forward is
checked against the composition bit for bit before anything is timed. Algorithmic bytes:
  forward    E 4F (gathered rows) + n_dst (R + 1) 4F (out) + E 8 (col_ind, edge_type) + n_dst 4 (row_ptr)
  backward   E 4F (gathered grad_out slots) + n_src 4F (grad_x) + E 16 (order, sorted target, edge_type, edge_scale)
the fraction is of 8 TB/s."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import PEAK, timed  # noqa: E402


def sub_blocks(row_ptr, col, et, R):
    """per relation r: (row_ptr_r, col_ind_r) of the edges of type r, their relative order kept"""
    import torch
    n_dst = row_ptr.numel() - 1
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=col.device), deg)
    out = []
    for r in range(R):
        keep = et == r
        ptr = torch.zeros(n_dst + 1, dtype=torch.int32, device=col.device)
        ptr[1:] = torch.cumsum(torch.bincount(dst[keep], minlength=n_dst), 0).to(torch.int32)
        out.append((ptr, col[keep].contiguous()))
    return out


def run_relations(R, row_ptr, col, n_src, dim, aggr, warmup, reps, gen):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.rel_aggregation import agg_concat_rel
    n_dst, E = row_ptr.numel() - 1, col.numel()
    et = torch.randint(0, R, (E,), device="cuda", generator=gen, dtype=torch.int32)
    x = torch.randn((n_src, dim), device="cuda", generator=gen).requires_grad_(True)
    G = torch.randn((n_dst, (R + 1) * dim), device="cuda", generator=gen)
    xd = x.detach()
    blocks = sub_blocks(row_ptr, col, et, R)

    def composed(rows):
        parts = [agg_concat(rows, p, c, aggr)[:, :dim] for p, c in blocks]
        return torch.cat(parts + [rows[:n_dst]], dim=1)

    out = agg_concat_rel(x, row_ptr, col, et, R, aggr)
    x2 = xd.clone().requires_grad_(True)
    cout = composed(x2)
    assert torch.equal(out.detach().view(torch.int32), cout.detach().view(torch.int32)), "fused != composition"
    fwd_ms = timed(lambda: agg_concat_rel(xd, row_ptr, col, et, R, aggr), warmup, reps)
    cf_ms = timed(lambda: composed(xd), warmup, reps)

    def bwd():
        x.grad = None
        torch.autograd.backward(out, G, retain_graph=True)

    def cbwd():
        x2.grad = None
        torch.autograd.backward(cout, G, retain_graph=True)
    bwd_ms = timed(bwd, warmup, reps)
    cb_ms = timed(cbwd, warmup, reps)
    rel = float((x.grad - x2.grad).norm() / x2.grad.norm().clamp(min=1e-30))
    assert rel < 1e-5, rel   # (the composition adds the R gradients of x in autograd's order: not the fused order)
    fwd_bytes = E * 4 * dim + n_dst * (R + 1) * 4 * dim + E * 8 + n_dst * 4
    bwd_bytes = E * 4 * dim + n_src * 4 * dim + E * 16
    res = {"relations": R, "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": dim, "aggr": aggr,
           "forward_ms": round(fwd_ms, 4), "backward_ms": round(bwd_ms, 4), "fwd_bwd_ms": round(fwd_ms + bwd_ms, 4),
           "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "backward_frac_8TBps": round(bwd_bytes / bwd_ms / 1e-3 / PEAK, 4),
           "fwd_bwd_frac_8TBps": round((fwd_bytes + bwd_bytes) / (fwd_ms + bwd_ms) / 1e-3 / PEAK, 4),
           "composed_forward_ms": round(cf_ms, 4), "composed_backward_ms": round(cb_ms, 4),
           "composed_fwd_bwd_ms": round(cf_ms + cb_ms, 4),
           "speedup_forward": round(cf_ms / fwd_ms, 2), "speedup_backward": round(cb_ms / bwd_ms, 2),
           "speedup_fwd_bwd": round((cf_ms + cb_ms) / (fwd_ms + bwd_ms), 2)}
    del x, x2, out, cout, G, blocks
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--relations", default="2,4,8", help="comma-separated numbers of relations")
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--aggr", default="mean")
    p.add_argument("--n-dst", type=int, default=333_334)
    p.add_argument("--fanout", type=int, default=30)
    p.add_argument("--n-src", type=int, default=2_000_000)
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_rgcn.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges

    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    col = torch.randint(0, a.n_src, (a.n_dst * a.fanout,), device="cuda", generator=gen, dtype=torch.int32)
    results = [run_relations(int(r), row_ptr, col, a.n_src, a.dim, a.aggr, a.warmup, a.reps, gen)
               for r in a.relations.split(",")]
    line = {"bench": "rgcn", "chunk_edges": chunk_edges(), "peak_Bps": PEAK, "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
