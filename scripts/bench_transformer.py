#!/usr/bin/env python3
"""Timing of the scaled dot-product attention aggregation (wholegraph_amd/torch/transformer_aggregation.py ->
csrc/kernels/tconv.hip) on one MI355X; prints ONE JSON line.

Shapes (those of scripts/bench_gatv2.py), H = 4 heads of F = 32 (H*F = 128), concat, norm_by_dim:
  a  uniform:   n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M
  b  power-law: the same with col_ind drawn from a truncated power law (s 0.8): hub sources with thousands of edges
  c  layer 0 of a BASELINE config 5 sample (1024 seeds, fan-outs 30,30)

Per shape, the median of `--reps` calls after `--warmup`: the forward and the full backward (all three gradients), and on
the same block in the same process the torch composite of the op (index_select, a scatter-amax / exp / index_add_ softmax,
index_add_; its backward through autograd) and mha_gat_v2_n2n. Algorithmic bytes (HF = H*F):
  forward    n_dst 4HF (query) + E (4 + 8HF + 4H) (col_ind, a key row, a value row, alpha) + n_dst 4HF (out)
  backward   target side E (4 + 8HF + 12H) (col_ind, a value row, a key row; alpha, da, ds) + n_dst 8HF (G, grad_query);
             source side E (8 + 8HF + 8H) (order, sorted_dst, G[d] and query[d]; alpha, ds) + n_src 8HF (grad_key,
             grad_value)
the fraction is of 8 TB/s. `--calls N` instead runs N forward + backward calls of shape a and nothing else (for a
rocprofv3 --kernel-trace --stats run of this script)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import PEAK, c5_layer0, powerlaw_ids, timed  # noqa: E402


def composite(key, query, value, row_ptr, col, H):
    import torch
    n_dst = row_ptr.numel() - 1
    F = key.shape[1] // H
    kv, qv, vv = key.view(-1, H, F), query.view(-1, H, F), value.view(-1, H, F)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=key.device), deg)
    col = col.long()
    l = (qv[dst] * kv[col]).sum(-1) / F ** 0.5
    m = torch.full((n_dst, H), -float("inf"), device=key.device).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=key.device).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=key.device).index_add_(0, dst, alpha[:, :, None] * vv[col])
    return o.reshape(n_dst, H * F)


def make_inputs(row_ptr, n_src, H, F):
    import torch
    n_dst, HF = row_ptr.numel() - 1, H * F
    gen = torch.Generator(device="cuda").manual_seed(3)
    key = torch.randn((n_src, HF), device="cuda", generator=gen).requires_grad_(True)
    query = torch.randn((n_dst, HF), device="cuda", generator=gen).requires_grad_(True)
    value = torch.randn((n_src, HF), device="cuda", generator=gen).requires_grad_(True)
    G = torch.randn((n_dst, HF), device="cuda", generator=gen)
    return key, query, value, G


def run_shape(name, row_ptr, col_ind, n_src, H, F, warmup, reps):
    import torch
    from wholegraph_amd.torch.gatv2_aggregation import mha_gat_v2_n2n
    from wholegraph_amd.torch.transformer_aggregation import mha_simple_n2n
    n_dst, E, HF = row_ptr.numel() - 1, col_ind.numel(), H * F
    key, query, value, G = make_inputs(row_ptr, n_src, H, F)
    out = mha_simple_n2n(key, query, value, row_ptr, col_ind, H)
    kd, qd, vd = key.detach(), query.detach(), value.detach()
    fwd_ms = timed(lambda: mha_simple_n2n(kd, qd, vd, row_ptr, col_ind, H), warmup, reps)

    def bwd():
        key.grad = query.grad = value.grad = None
        torch.autograd.backward(out, G, retain_graph=True)
    bwd_ms = timed(bwd, warmup, reps)

    # mha_gat_v2_n2n on the same block (h_src = key, h_dst = query, att [H * F])
    gs, gd = kd.clone().requires_grad_(True), qd.clone().requires_grad_(True)
    gatt = (0.2 * vd[0]).clone().requires_grad_(True)
    gout = mha_gat_v2_n2n(gs, gd, gatt, row_ptr, col_ind, H)
    gf_ms = timed(lambda: mha_gat_v2_n2n(kd, qd, gatt.detach(), row_ptr, col_ind, H), warmup, reps)

    def gbwd():
        gs.grad = gd.grad = gatt.grad = None
        torch.autograd.backward(gout, G, retain_graph=True)
    gb_ms = timed(gbwd, warmup, reps)
    del gs, gd, gatt, gout

    cf_ms = timed(lambda: composite(kd, qd, vd, row_ptr, col_ind, H), warmup, reps)
    k2, q2, v2 = (t.clone().requires_grad_(True) for t in (kd, qd, vd))
    cout = composite(k2, q2, v2, row_ptr, col_ind, H)

    def cbwd():
        k2.grad = q2.grad = v2.grad = None
        torch.autograd.backward(cout, G, retain_graph=True)
    cb_ms = timed(cbwd, warmup, reps)

    def rel(a_, b_):
        return float((a_ - b_).norm() / b_.norm().clamp(min=1e-30))
    assert rel(out.detach(), cout.detach()) < 1e-5
    bwd()
    cbwd()
    assert rel(key.grad, k2.grad) < 1e-4 and rel(query.grad, q2.grad) < 1e-4 and rel(value.grad, v2.grad) < 1e-4

    fwd_bytes = n_dst * 4 * HF + E * (4 + 8 * HF + 4 * H) + n_dst * 4 * HF
    bwd_bytes = E * (12 + 16 * HF + 20 * H) + n_dst * 8 * HF + n_src * 8 * HF
    counts = torch.bincount(col_ind.long(), minlength=n_src)
    res = {"shape": name, "n_dst": n_dst, "n_src": n_src, "edges": E, "heads": H, "dim": F,
           "max_edges_per_source": int(counts.max()),
           "forward_ms": round(fwd_ms, 4), "forward_GBps": round(fwd_bytes / fwd_ms / 1e6, 1),
           "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "backward_ms": round(bwd_ms, 4), "backward_GBps": round(bwd_bytes / bwd_ms / 1e6, 1),
           "backward_frac_8TBps": round(bwd_bytes / bwd_ms / 1e-3 / PEAK, 4),
           "gatv2_forward_ms": round(gf_ms, 4), "gatv2_backward_ms": round(gb_ms, 4),
           "forward_over_gatv2": round(fwd_ms / gf_ms, 3), "backward_over_gatv2": round(bwd_ms / gb_ms, 3),
           "torch_forward_ms": round(cf_ms, 4), "torch_backward_ms": round(cb_ms, 4),
           "speedup_forward_vs_torch": round(cf_ms / fwd_ms, 2), "speedup_backward_vs_torch": round(cb_ms / bwd_ms, 2)}
    del key, query, value, out, G, k2, q2, v2, cout
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--heads", type=int, default=4)
    p.add_argument("--dim", type=int, default=32, help="F, columns per head")
    p.add_argument("--n-dst", type=int, default=333_334)
    p.add_argument("--fanout", type=int, default=30)
    p.add_argument("--n-src", type=int, default=2_000_000)
    p.add_argument("--nodes", type=int, default=111_059_956, help="shape c: graph nodes (bench.py sample_gather default)")
    p.add_argument("--shapes", default="a,b,c")
    p.add_argument("--out", help="also write the JSON line to this file")
    p.add_argument("--calls", type=int, default=0,
                   help="run this many forward + backward calls of shape a and nothing else (under an outer profiler)")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_transformer.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges

    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    E = a.n_dst * a.fanout
    if a.calls > 0:
        from wholegraph_amd.torch.transformer_aggregation import mha_simple_n2n
        col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
        key, query, value, G = make_inputs(row_ptr, a.n_src, a.heads, a.dim)
        for _ in range(a.calls):
            key.grad = query.grad = value.grad = None
            mha_simple_n2n(key, query, value, row_ptr, col, a.heads).backward(G)
        torch.cuda.synchronize()
        print(json.dumps({"bench": "transformer", "calls": a.calls, "shape": "a_uniform"}), flush=True)
        return
    results = []
    for shape in a.shapes.split(","):
        if shape == "a":
            col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
            results.append(run_shape("a_uniform", row_ptr, col, a.n_src, a.heads, a.dim, a.warmup, a.reps))
        elif shape == "b":
            col = powerlaw_ids(a.n_src, E, 0.8, gen)
            results.append(run_shape("b_powerlaw", row_ptr, col, a.n_src, a.heads, a.dim, a.warmup, a.reps))
        elif shape == "c":
            rp, ci, n_src = c5_layer0(wgth, comm, a.nodes, 29, 1024, [30, 30])
            results.append(run_shape("c_c5_layer0", rp, ci, n_src, a.heads, a.dim, a.warmup, a.reps))
    line = {"bench": "transformer", "chunk_edges": chunk_edges(), "peak_Bps": PEAK, "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
