#!/usr/bin/env python3
"""Timing of the edge dot product (wholegraph_amd/torch/edge_dot.py -> csrc/kernels/edot.hip) on one MI355X against the
torch composite it replaces; prints ONE JSON line.

Shapes (a, b, c: those of scripts/bench_transformer.py), F = 128:
  a  uniform:   n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M
  b  power-law: the same with col_ind drawn from a truncated power law (s 0.8): hub sources with thousands of edges
  c  layer 0 of a BASELINE config 5 sample (1024 seeds, fan-outs 30,30)
  d  the block Node2Vec.sample builds for 1000 walks of 80 steps, W = 5, K = 5, on a power-law graph of `--d-nodes` nodes in
     CHUNKED WholeMemory; with it the time of skipgram_block on that batch, of the whole sample() and of one training step
     (sample, loss, backward, sparse SGD step), and the builder's share of the step

Per shape, the median of `--reps` calls after `--warmup`, in one process: the op's forward and forward + backward (both
gradients), and the composite's (index_select, multiply, sum(-1); its backward through autograd). Algorithmic bytes:
  forward               n_dst 4F (x_dst) + E (8 + 4F) (col_ind, a source row, the score)
  per-target backward   E (8 + 4F) (col_ind, g, a source row) + n_dst 4F (grad_dst)
  per-source backward   E (12 + 4F) (order, sorted_dst, g, a target row) + n_src 4F (grad_src)
the fraction is of 8 TB/s. The backward's time includes the id sort of col_ind, which the byte model leaves out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import PEAK, c5_layer0, powerlaw_ids, timed  # noqa: E402


def composite(x_src, x_dst, row_ptr, col):
    import torch
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(deg.numel(), device=x_src.device), deg)
    return (x_dst.index_select(0, dst) * x_src.index_select(0, col.long())).sum(-1)


def run_shape(name, row_ptr, col_ind, n_src, F, warmup, reps):
    import torch
    from wholegraph_amd.torch.edge_dot import edge_dot_n2n
    n_dst, E = row_ptr.numel() - 1, col_ind.numel()
    gen = torch.Generator(device="cuda").manual_seed(3)
    xs = torch.randn((n_src, F), device="cuda", generator=gen)
    xd = torch.randn((n_dst, F), device="cuda", generator=gen)
    G = torch.randn((E,), device="cuda", generator=gen)

    def both(fn):
        a, b = xs.clone().requires_grad_(True), xd.clone().requires_grad_(True)

        def step():
            a.grad = b.grad = None
            fn(a, b, row_ptr, col_ind).backward(G)
        return step, a, b

    fwd_ms = timed(lambda: edge_dot_n2n(xs, xd, row_ptr, col_ind), warmup, reps)
    step, a1, b1 = both(edge_dot_n2n)
    full_ms = timed(step, warmup, reps)
    cf_ms = timed(lambda: composite(xs, xd, row_ptr, col_ind), warmup, reps)
    cstep, a2, b2 = both(composite)
    cfull_ms = timed(cstep, warmup, reps)

    def rel(p, q):
        return float((p - q).norm() / q.norm().clamp(min=1e-30))
    assert rel(edge_dot_n2n(xs, xd, row_ptr, col_ind), composite(xs, xd, row_ptr, col_ind)) < 1e-5
    assert rel(a1.grad, a2.grad) < 1e-4 and rel(b1.grad, b2.grad) < 1e-4

    fwd_bytes = n_dst * 4 * F + E * (8 + 4 * F)
    bwd_bytes = E * (8 + 4 * F) + n_dst * 4 * F + E * (12 + 4 * F) + n_src * 4 * F
    bwd_ms = full_ms - fwd_ms
    counts = torch.bincount(col_ind.long(), minlength=n_src)
    res = {"shape": name, "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": F,
           "max_edges_per_source": int(counts.max()),
           "forward_ms": round(fwd_ms, 4), "forward_GBps": round(fwd_bytes / fwd_ms / 1e6, 1),
           "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "forward_backward_ms": round(full_ms, 4),
           "forward_backward_frac_8TBps": round((fwd_bytes + bwd_bytes) / full_ms / 1e-3 / PEAK, 4),
           "backward_ms_by_difference": round(bwd_ms, 4),
           "torch_forward_ms": round(cf_ms, 4), "torch_forward_backward_ms": round(cfull_ms, 4),
           "speedup_forward_vs_torch": round(cf_ms / fwd_ms, 2),
           "speedup_forward_backward_vs_torch": round(cfull_ms / full_ms, 2)}
    del xs, xd, G, a1, b1, a2, b2
    torch.cuda.empty_cache()
    return res


def node2vec_shape(wgth, comm, a):
    """shape d: the model's own batch, and where a training step's time goes"""
    import torch
    from wholegraph_amd.torch.skipgram import skipgram_block
    gen = torch.Generator(device="cuda").manual_seed(5)
    n = a.d_nodes
    row = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.randint(1, 2 * a.d_degree, (n,), device="cuda", generator=gen), 0, out=row[1:])
    edges = int(row[-1])
    wrow = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [n + 1], torch.int64, [1])
    wcol = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [edges], torch.int64, [1])
    wrow.get_local_tensor()[0].copy_(row)
    wcol.get_local_tensor()[0].copy_(powerlaw_ids(n, edges, 0.8, gen).long())
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [n, a.dim])
    emb.get_embedding_tensor().get_local_tensor()[0].normal_(0.0, 0.1, generator=gen)
    opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    model = wgth.Node2Vec(g, emb, walk_length=80, window=5, num_negatives=5)
    starts = torch.randint(0, n, (1000,), device="cuda", generator=gen)
    batch = model.sample(starts, random_seed=7)
    negatives = g.negative_sample(batch.center_ids, 5, random_seed=8)
    seeds = iter(range(100, 10000))

    def step():
        model(starts, random_seed=next(seeds)).backward()
        opt.step(100.0)
    builder_ms = timed(lambda: skipgram_block(batch.walks, 5, negatives), a.warmup, a.reps)
    sample_ms = timed(lambda: model.sample(starts, random_seed=next(seeds)), a.warmup, a.reps)
    step_ms = timed(step, a.warmup, a.reps)
    res = run_shape("d_node2vec_batch", batch.row_ptr, batch.col_ind, int(batch.unique_ctx.numel()), a.dim, a.warmup, a.reps)
    res.update({"graph_nodes": n, "graph_edges": edges, "walks": 1000, "walk_length": 80, "window": 5, "num_negatives": 5,
                "skipgram_block_ms": round(builder_ms, 4), "sample_ms": round(sample_ms, 4),
                "train_step_ms": round(step_ms, 4), "builder_share_of_step": round(builder_ms / step_ms, 4)})
    wgth.destroy_wholememory_optimizer(opt)
    wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--dim", type=int, default=128, help="F, columns of a row")
    p.add_argument("--n-dst", type=int, default=333_334)
    p.add_argument("--fanout", type=int, default=30)
    p.add_argument("--n-src", type=int, default=2_000_000)
    p.add_argument("--nodes", type=int, default=111_059_956, help="shape c: graph nodes (bench.py sample_gather default)")
    p.add_argument("--d-nodes", type=int, default=1_000_000, help="shape d: graph nodes")
    p.add_argument("--d-degree", type=int, default=15, help="shape d: mean out-degree")
    p.add_argument("--shapes", default="a,b,c,d")
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_edge_dot.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges

    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    E = a.n_dst * a.fanout
    results = []
    for shape in a.shapes.split(","):
        if shape == "a":
            col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
            results.append(run_shape("a_uniform", row_ptr, col, a.n_src, a.dim, a.warmup, a.reps))
        elif shape == "b":
            col = powerlaw_ids(a.n_src, E, 0.8, gen)
            results.append(run_shape("b_powerlaw", row_ptr, col, a.n_src, a.dim, a.warmup, a.reps))
        elif shape == "c":
            rp, ci, n_src = c5_layer0(wgth, comm, a.nodes, 29, 1024, [30, 30])
            results.append(run_shape("c_c5_layer0", rp, ci, n_src, a.dim, a.warmup, a.reps))
        elif shape == "d":
            results.append(node2vec_shape(wgth, comm, a))
    line = {"bench": "edge_dot", "chunk_edges": chunk_edges(), "peak_Bps": PEAK, "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
