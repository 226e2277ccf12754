#!/usr/bin/env python3
"""Timing of the GAT attention aggregation (wholegraph_amd/torch/gat_aggregation.py -> csrc/kernels/gat.hip) on one
MI355X; prints ONE JSON line.

Shapes (those of scripts/bench_sage_agg.py), H = 4 heads of F = 32 (H*F = 128), concat:
  a  uniform:   n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M
  b  power-law: the same with col_ind drawn from a truncated power law (s 0.8): hub sources with thousands of edges
  c  layer 0 of a BASELINE config 5 sample (1024 seeds, fan-outs 30,30)

Per shape: the forward (scores + attention + row pass), the full backward, and the backward split by kernel from device
times (torch.profiler): the edge kernel, the edge index (id sort + gat_bwd_prep_kernel), the fold (gat_bwd_chunk_kernel +
gat_bwd_fold_kernel) and grad_att. Algorithmic bytes (HF = H*F):
  forward       n_src 4HF (scores) + E (4 + 8H + 4HF) + n_dst 4HF + (n_src + n_dst) 4H
  edge + fold   E (12 + 8HF + 12H) + n_dst (4HF + 4H) + n_src (4HF + 4H)
the fraction is of 8 TB/s. The torch composite of the same op in the same process (index_select, a scatter-max / exp /
index_add_ softmax, index_add_; its backward through autograd) and agg_concat's forward on the same block give the ratios."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import PEAK, c5_layer0, powerlaw_ids, timed  # noqa: E402


def kernel_split(fn, reps):
    """mean device ms per call of the backward's kernel groups, from torch.profiler's kernel records; None when the
    profiler records no kernel of this library"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
    except Exception as e:   # (the split is then left to a rocprofv3 --kernel-trace --stats run of this script)
        print("kernel_split: torch.profiler failed: %s" % e, file=sys.stderr)
        return None
    t = {"edge": 0.0, "fold": 0.0, "att": 0.0, "index": 0.0}
    seen = False
    for ev in prof.events():
        if ev.device_type != torch.autograd.DeviceType.CUDA:
            continue
        name = ev.name
        d = getattr(ev, "device_time", None)
        if d is None:
            d = getattr(ev, "cuda_time", 0.0)
        if "gat_bwd_edge_kernel" in name:
            t["edge"] += d
            seen = True
        elif "gat_bwd_chunk_kernel" in name or "gat_bwd_fold_kernel" in name:
            t["fold"] += d
        elif "gat_att_" in name:
            t["att"] += d
        elif "elementwise" not in name.lower() and "fill" not in name.lower() and "gat_" not in name:
            t["index"] += d   # the id sort's kernels (gat_bwd_prep_kernel is counted below)
        if "gat_bwd_prep_kernel" in name:
            t["index"] += d
    if not seen:
        return None
    return {k: v / 1000.0 / reps for k, v in t.items()}


def composite(h, att, row_ptr, col, H, slope):
    import torch
    n_dst = row_ptr.numel() - 1
    F = h.shape[1] // H
    hv, a = h.view(-1, H, F), att.view(2, H, F)
    s_src = (hv * a[0]).sum(-1)
    s_dst = (hv[:n_dst] * a[1]).sum(-1)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=h.device), deg)
    col = col.long()
    l = torch.nn.functional.leaky_relu(s_src[col] + s_dst[dst], slope)
    m = torch.full((n_dst, H), -float("inf"), device=h.device).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=h.device).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=h.device).index_add_(0, dst, alpha[:, :, None] * hv[col])
    return o.reshape(n_dst, H * F)


def run_shape(name, row_ptr, col_ind, n_src, H, F, warmup, reps, split_kernels=True):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    n_dst, E, HF = row_ptr.numel() - 1, col_ind.numel(), H * F
    gen = torch.Generator(device="cuda").manual_seed(3)
    h = torch.randn((n_src, HF), device="cuda", generator=gen).requires_grad_(True)
    att = (0.2 * torch.randn((2 * HF,), device="cuda", generator=gen)).requires_grad_(True)
    out = mha_gat_n2n(h, att, row_ptr, col_ind, H)
    G = torch.randn(tuple(out.shape), device="cuda", generator=gen)
    hd, ad = h.detach(), att.detach()

    fwd_ms = timed(lambda: mha_gat_n2n(hd, ad, row_ptr, col_ind, H), warmup, reps)
    agg_ms = timed(lambda: agg_concat(hd, row_ptr, col_ind, "sum"), warmup, reps)

    def bwd():
        h.grad = att.grad = None
        torch.autograd.backward(out, G, retain_graph=True)
    bwd_ms = timed(bwd, warmup, reps)
    split = kernel_split(bwd, max(3, reps // 2)) if split_kernels else None

    cf_ms = timed(lambda: composite(hd, ad, row_ptr, col_ind, H, 0.2), warmup, reps)
    h2, a2 = hd.clone().requires_grad_(True), ad.clone().requires_grad_(True)
    cout = composite(h2, a2, row_ptr, col_ind, H, 0.2)

    def cbwd():
        h2.grad = a2.grad = None
        torch.autograd.backward(cout, G, retain_graph=True)
    cb_ms = timed(cbwd, warmup, reps)

    def rel(a_, b_):
        return float((a_ - b_).norm() / b_.norm().clamp(min=1e-30))
    assert rel(out.detach(), cout.detach()) < 1e-5
    bwd()
    cbwd()
    assert rel(h.grad, h2.grad) < 1e-4 and rel(att.grad, a2.grad) < 1e-4

    fwd_bytes = n_src * 4 * HF + E * (4 + 8 * H + 4 * HF) + n_dst * 4 * HF + (n_src + n_dst) * 4 * H
    bwd_bytes = E * (12 + 8 * HF + 12 * H) + n_dst * (4 * HF + 4 * H) + n_src * (4 * HF + 4 * H)
    counts = torch.bincount(col_ind.long(), minlength=n_src)
    res = {"shape": name, "n_dst": n_dst, "n_src": n_src, "edges": E, "heads": H, "dim": F,
           "max_edges_per_source": int(counts.max()),
           "forward_ms": round(fwd_ms, 4), "forward_GBps": round(fwd_bytes / fwd_ms / 1e6, 1),
           "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "agg_concat_forward_ms": round(agg_ms, 4), "forward_over_agg_concat": round(fwd_ms / agg_ms, 3),
           "backward_ms": round(bwd_ms, 4),
           "torch_forward_ms": round(cf_ms, 4), "torch_backward_ms": round(cb_ms, 4),
           "speedup_forward_vs_torch": round(cf_ms / fwd_ms, 2), "speedup_backward_vs_torch": round(cb_ms / bwd_ms, 2)}
    if split is not None:
        ef = split["edge"] + split["fold"]
        res.update({k + "_ms": round(v, 4) for k, v in split.items()})
        res.update({"edge_fold_GBps": round(bwd_bytes / ef / 1e6, 1),
                    "edge_fold_frac_8TBps": round(bwd_bytes / ef / 1e-3 / PEAK, 4)})
    del h, att, out, G, h2, a2, cout
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
    p.add_argument("--no-kernel-split", action="store_true",
                   help="skip the torch.profiler split of the backward (when an outer profiler such as rocprofv3 traces the run)")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_gat.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import node_chunk

    results = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    E = a.n_dst * a.fanout
    split = not a.no_kernel_split
    for shape in a.shapes.split(","):
        if shape == "a":
            col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
            results.append(run_shape("a_uniform", row_ptr, col, a.n_src, a.heads, a.dim, a.warmup, a.reps, split))
        elif shape == "b":
            col = powerlaw_ids(a.n_src, E, 0.8, gen)
            results.append(run_shape("b_powerlaw", row_ptr, col, a.n_src, a.heads, a.dim, a.warmup, a.reps, split))
        elif shape == "c":
            rp, ci, n_src = c5_layer0(wgth, comm, a.nodes, 29, 1024, [30, 30])
            results.append(run_shape("c_c5_layer0", rp, ci, n_src, a.heads, a.dim, a.warmup, a.reps, split))
    line = {"bench": "gat", "chunk_edges": chunk_edges(), "node_chunk": node_chunk(), "peak_Bps": PEAK,
            "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
