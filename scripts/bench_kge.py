#!/usr/bin/env python3
"""Timing of the relation-typed edge score (wholegraph_amd/torch/kge_score.py -> csrc/kernels/kge.hip) on one MI355X
against the torch composite it replaces; prints ONE JSON line (and writes it to profiles/kge_bench.json with --out).

Shapes, F = 128, R = 64 relations, the relation repeated along a target's row as kge_block builds it:
  a  uniform:   n_dst 262,144 triples x (1 + 15 negatives) edges (E = 4.2 M), n_src 1 M distinct tails
  b  power-law: the same with col_ind drawn from a truncated power law (s 0.8): hub tails with thousands of edges

Per shape and model, the median of `--reps` calls after `--warmup`, in one process: the op's forward and forward + backward
(the three gradients), and the composite's (three index_selects, the model's formula, sum(-1); its backward through autograd).
Algorithmic bytes (the relation table, R 4F bytes, stays in L2 and is left out):
  forward               n_dst 4F (the target's row) + E (12 + 4F) (col_ind, edge_type, the far row, the score)
  per-target backward   E (16 + 4F) (col_ind, edge_type, g, the far row; + 4 for n in the l2 models) + n_dst 8F
  per-source backward   E (16 + 4F) (order, sorted_dst, edge_type, g, the target's row) + n_src 8F
  per-relation backward E (16 + 8F) (order, sorted_dst, col_ind, g, both rows) + the partial rows, E / C 8F
the fraction is of 8 TB/s. The backward's time includes the two id sorts, which the byte model leaves out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import PEAK, powerlaw_ids, timed  # noqa: E402

MODELS = ("distmult", "transe_l1", "transe_l2", "complex", "rotate")


def composite(model, x_src, x_dst, rel, row_ptr, col, et):
    """the plain torch formula of the model, head = the target's row"""
    import torch
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    h = x_dst.index_select(0, torch.repeat_interleave(torch.arange(deg.numel(), device=x_src.device), deg))
    t, r = x_src.index_select(0, col.long()), rel.index_select(0, et.long())
    if model == "distmult":
        return (h * r * t).sum(-1)
    if model == "transe_l1":
        return -(h + r - t).abs().sum(-1)
    if model == "transe_l2":
        return -(h + r - t).pow(2).sum(-1).sqrt()
    D = h.shape[1] // 2
    u_re = h[:, :D] * r[:, :D] - h[:, D:] * r[:, D:]
    u_im = h[:, :D] * r[:, D:] + h[:, D:] * r[:, :D]
    if model == "complex":
        return (u_re * t[:, :D] + u_im * t[:, D:]).sum(-1)
    return -((u_re - t[:, :D]).pow(2) + (u_im - t[:, D:]).pow(2)).sum(-1).sqrt()


def run_shape(name, model, row_ptr, col, et, n_src, R, F, C, warmup, reps):
    import torch
    from wholegraph_amd.torch.kge_score import kge_score_n2n
    n_dst, E = row_ptr.numel() - 1, col.numel()
    gen = torch.Generator(device="cuda").manual_seed(3)
    xs = torch.randn((n_src, F), device="cuda", generator=gen)
    xd = torch.randn((n_dst, F), device="cuda", generator=gen)
    rel = torch.randn((R, F), device="cuda", generator=gen)
    G = torch.randn((E,), device="cuda", generator=gen)

    def op(a, b, c):
        return kge_score_n2n(a, b, c, row_ptr, col, et, model=model)

    def ref(a, b, c):
        return composite(model, a, b, c, row_ptr, col, et)

    def all_three(fn):
        leaves = [t.clone().requires_grad_(True) for t in (xs, xd, rel)]

        def step():
            for t in leaves:
                t.grad = None
            fn(*leaves).backward(G)
        return step, leaves

    fwd_ms = timed(lambda: op(xs, xd, rel), warmup, reps)
    step, mine = all_three(op)
    full_ms = timed(step, warmup, reps)
    cf_ms = timed(lambda: ref(xs, xd, rel), warmup, reps)
    cstep, theirs = all_three(ref)
    cfull_ms = timed(cstep, warmup, reps)

    def close(p, q):
        return float((p - q).norm() / q.norm().clamp(min=1e-30))
    assert close(op(xs, xd, rel), ref(xs, xd, rel)) < 1e-5
    assert all(close(a.grad, b.grad) < 1e-4 for a, b in zip(mine, theirs))

    fwd_bytes = n_dst * 4 * F + E * (12 + 4 * F)
    bwd_bytes = E * (16 + 4 * F) + n_dst * 8 * F + E * (16 + 4 * F) + n_src * 8 * F + E * (16 + 8 * F) + (E // C) * 8 * F
    res = {"shape": name, "model": model, "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": F, "relations": R,
           "forward_ms": round(fwd_ms, 4), "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "forward_backward_ms": round(full_ms, 4),
           "forward_backward_frac_8TBps": round((fwd_bytes + bwd_bytes) / full_ms / 1e-3 / PEAK, 4),
           "backward_ms_by_difference": round(full_ms - fwd_ms, 4),
           "torch_forward_ms": round(cf_ms, 4), "torch_forward_backward_ms": round(cfull_ms, 4),
           "speedup_forward_vs_torch": round(cf_ms / fwd_ms, 2),
           "speedup_forward_backward_vs_torch": round(cfull_ms / full_ms, 2)}
    del xs, xd, rel, G, mine, theirs
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--dim", type=int, default=128, help="F, columns of a row")
    p.add_argument("--n-dst", type=int, default=262_144)
    p.add_argument("--negatives", type=int, default=15)
    p.add_argument("--n-src", type=int, default=1_000_000)
    p.add_argument("--relations", type=int, default=64)
    p.add_argument("--shapes", default="a,b")
    p.add_argument("--models", default=",".join(MODELS))
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_kge.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges

    gen = torch.Generator(device="cuda").manual_seed(2)
    width = a.negatives + 1
    row_ptr = torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * width
    E = a.n_dst * width
    et = torch.randint(0, a.relations, (a.n_dst,), device="cuda", generator=gen, dtype=torch.int32).repeat_interleave(width)
    results = []
    for shape in a.shapes.split(","):
        if shape == "a":
            name, col = "a_uniform", torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
        else:
            name, col = "b_powerlaw", powerlaw_ids(a.n_src, E, 0.8, gen)
        for model in a.models.split(","):
            results.append(run_shape(name, model, row_ptr, col, et, a.n_src, a.relations, a.dim, chunk_edges(), a.warmup,
                                     a.reps))
    line = {"bench": "kge_score", "chunk_edges": chunk_edges(), "peak_Bps": PEAK, "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
