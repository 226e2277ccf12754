#!/usr/bin/env python3
"""Timing of the GATv2 attention aggregation (wholegraph_amd/torch/gatv2_aggregation.py -> csrc/kernels/gatv2.hip) on one
MI355X; prints ONE JSON line.

Shapes (those of scripts/bench_gat.py), H = 4 heads of F = 32 (H*F = 128), concat:
  a  uniform:   n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M
  b  power-law: the same with col_ind drawn from a truncated power law (s 0.8): hub sources with thousands of edges
  c  layer 0 of a BASELINE config 5 sample (1024 seeds, fan-outs 30,30)

Per shape, the median of `--reps` calls after `--warmup`: the forward and the full backward (all three gradients), and on
the same block in the same process the torch composite of the op (index_select, a scatter-max / exp / index_add_ softmax,
index_add_; its backward through autograd) and mha_gat_n2n. Algorithmic bytes (HF = H*F):
  forward    n_dst 4HF (h_dst) + E (4 + 4HF + 4H) + n_dst 4HF (out); + E 4HF if the second row pass misses cache
  backward   GAT's edge + fold model, E (12 + 8HF + 12H) + n_dst (4HF + 4H) + n_src (4HF + 4H), plus two row reads per
             edge (G[d] and h_dst[d] in the per-source pass): + E 8HF
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


def composite(hs, hd, att, row_ptr, col, H, slope):
    import torch
    n_dst = row_ptr.numel() - 1
    F = hs.shape[1] // H
    hv, dv, a = hs.view(-1, H, F), hd.view(-1, H, F), att.view(H, F)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=hs.device), deg)
    col = col.long()
    l = (torch.nn.functional.leaky_relu(hv[col] + dv[dst], slope) * a).sum(-1)
    m = torch.full((n_dst, H), -float("inf"), device=hs.device).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=hs.device).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=hs.device).index_add_(0, dst, alpha[:, :, None] * hv[col])
    return o.reshape(n_dst, H * F)


def make_inputs(row_ptr, n_src, H, F):
    import torch
    n_dst, HF = row_ptr.numel() - 1, H * F
    gen = torch.Generator(device="cuda").manual_seed(3)
    hs = torch.randn((n_src, HF), device="cuda", generator=gen).requires_grad_(True)
    hd = torch.randn((n_dst, HF), device="cuda", generator=gen).requires_grad_(True)
    att = (0.2 * torch.randn((HF,), device="cuda", generator=gen)).requires_grad_(True)
    G = torch.randn((n_dst, HF), device="cuda", generator=gen)
    return hs, hd, att, G


def run_shape(name, row_ptr, col_ind, n_src, H, F, warmup, reps):
    import torch
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    from wholegraph_amd.torch.gatv2_aggregation import mha_gat_v2_n2n
    n_dst, E, HF = row_ptr.numel() - 1, col_ind.numel(), H * F
    hs, hd, att, G = make_inputs(row_ptr, n_src, H, F)
    out = mha_gat_v2_n2n(hs, hd, att, row_ptr, col_ind, H)
    hsd, hdd, ad = hs.detach(), hd.detach(), att.detach()
    fwd_ms = timed(lambda: mha_gat_v2_n2n(hsd, hdd, ad, row_ptr, col_ind, H), warmup, reps)

    def bwd():
        hs.grad = hd.grad = att.grad = None
        torch.autograd.backward(out, G, retain_graph=True)
    bwd_ms = timed(bwd, warmup, reps)

    # mha_gat_n2n on the same block (att [2, H, F])
    gh = hsd.clone().requires_grad_(True)
    gatt = torch.cat([ad, ad]).requires_grad_(True)
    gout = mha_gat_n2n(gh, gatt, row_ptr, col_ind, H)
    gf_ms = timed(lambda: mha_gat_n2n(hsd, gatt.detach(), row_ptr, col_ind, H), warmup, reps)

    def gbwd():
        gh.grad = gatt.grad = None
        torch.autograd.backward(gout, G, retain_graph=True)
    gb_ms = timed(gbwd, warmup, reps)
    del gh, gatt, gout

    cf_ms = timed(lambda: composite(hsd, hdd, ad, row_ptr, col_ind, H, 0.2), warmup, reps)
    hs2, hd2, a2 = (t.clone().requires_grad_(True) for t in (hsd, hdd, ad))
    cout = composite(hs2, hd2, a2, row_ptr, col_ind, H, 0.2)

    def cbwd():
        hs2.grad = hd2.grad = a2.grad = None
        torch.autograd.backward(cout, G, retain_graph=True)
    cb_ms = timed(cbwd, warmup, reps)

    def rel(a_, b_):
        return float((a_ - b_).norm() / b_.norm().clamp(min=1e-30))
    assert rel(out.detach(), cout.detach()) < 1e-5
    bwd()
    cbwd()
    assert rel(hs.grad, hs2.grad) < 1e-4 and rel(hd.grad, hd2.grad) < 1e-4 and rel(att.grad, a2.grad) < 1e-4

    fwd_bytes = n_dst * 4 * HF + E * (4 + 4 * HF + 4 * H) + n_dst * 4 * HF
    bwd_bytes = E * (12 + 8 * HF + 12 * H) + n_dst * (4 * HF + 4 * H) + n_src * (4 * HF + 4 * H) + E * 8 * HF
    counts = torch.bincount(col_ind.long(), minlength=n_src)
    res = {"shape": name, "n_dst": n_dst, "n_src": n_src, "edges": E, "heads": H, "dim": F,
           "max_edges_per_source": int(counts.max()),
           "forward_ms": round(fwd_ms, 4), "forward_GBps": round(fwd_bytes / fwd_ms / 1e6, 1),
           "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "forward_frac_8TBps_two_row_passes": round((fwd_bytes + E * 4 * HF) / fwd_ms / 1e-3 / PEAK, 4),
           "backward_ms": round(bwd_ms, 4), "backward_GBps": round(bwd_bytes / bwd_ms / 1e6, 1),
           "backward_frac_8TBps": round(bwd_bytes / bwd_ms / 1e-3 / PEAK, 4),
           "gat_forward_ms": round(gf_ms, 4), "gat_backward_ms": round(gb_ms, 4),
           "forward_over_gat": round(fwd_ms / gf_ms, 3), "backward_over_gat": round(bwd_ms / gb_ms, 3),
           "torch_forward_ms": round(cf_ms, 4), "torch_backward_ms": round(cb_ms, 4),
           "speedup_forward_vs_torch": round(cf_ms / fwd_ms, 2), "speedup_backward_vs_torch": round(cb_ms / bwd_ms, 2)}
    del hs, hd, att, out, G, hs2, hd2, a2, cout
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
    assert torch.cuda.is_available(), "bench_gatv2.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import node_chunk

    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    E = a.n_dst * a.fanout
    if a.calls > 0:
        from wholegraph_amd.torch.gatv2_aggregation import mha_gat_v2_n2n
        col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
        hs, hd, att, G = make_inputs(row_ptr, a.n_src, a.heads, a.dim)
        for _ in range(a.calls):
            hs.grad = hd.grad = att.grad = None
            mha_gat_v2_n2n(hs, hd, att, row_ptr, col, a.heads).backward(G)
        torch.cuda.synchronize()
        print(json.dumps({"bench": "gatv2", "calls": a.calls, "shape": "a_uniform"}), flush=True)
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
    line = {"bench": "gatv2", "chunk_edges": chunk_edges(), "node_chunk": node_chunk(), "peak_Bps": PEAK,
            "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
