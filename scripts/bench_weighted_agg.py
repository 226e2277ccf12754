#!/usr/bin/env python3
"""Timing of the edge-weighted neighbour aggregation (wholegraph_amd/torch/weighted_aggregation.py ->
csrc/kernels/agg_weighted.hip) on one MI355X; prints ONE JSON line.

Shapes a / b / c, F, "mean", warm-up and repetitions as scripts/bench_sage_agg.py (whose block builders are used). Per
shape, in one process and on one block:
  * the weighted op: forward, backward into x only, backward into x and w, backward into w only;
  * unweighted agg_concat (forward, backward) with the min and max of its repetitions — its own run-to-run spread;
  * the torch composite a user had to write without the op: (x[col] * w[:, None]) + index_add_ + mean + cat, forward, and
    backward through autograd with and without a gradient for w.
Per-kernel device times of the backward (torch.profiler): the fold (aggw_bwd_chunk_kernel + aggw_bwd_fold_kernel) and
aggw_bwd_weight_kernel. Algorithmic bytes: forward E(8 + 4F) + n_dst(4 + 12F); fold E(12 + 4F) + n_src 4F + n_dst 4F; weight
kernel E(12 + 4F) + n_dst 4F (each grad_out row counted once); fractions are of 8 TB/s.

Gates (reported as booleans, never tuned away): every weighted time below the composite's; weighted forward and weighted
grad_x backward at most (byte ratio of the two ops) x (agg_concat's max / median over its timed calls) x agg_concat."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_sage_agg as base   # noqa: E402

PEAK = base.PEAK


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def kernel_ms(fn, reps):
    """mean device ms per call of (fold kernels, weight kernel) from torch.profiler; None when it records none of them"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
    except Exception as e:   # (the split is then left to a rocprofv3 --kernel-trace --stats run of this script)
        print("kernel_ms: torch.profiler failed: %s" % e, file=sys.stderr)
        return None
    fold = weight = 0.0
    for ev in prof.events():
        if ev.device_type != torch.autograd.DeviceType.CUDA:
            continue
        t = getattr(ev, "device_time", None)
        if t is None:
            t = getattr(ev, "cuda_time", 0.0)
        if "aggw_bwd_chunk_kernel" in ev.name or "aggw_bwd_fold_kernel" in ev.name:
            fold += t
        elif "aggw_bwd_weight_kernel" in ev.name:
            weight += t
    if fold == 0.0 and weight == 0.0:
        return None
    return fold / 1000.0 / reps, weight / 1000.0 / reps


def run_shape(name, row_ptr, col_ind, n_src, dim, warmup, reps, split_kernels=True):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    n_dst, E = row_ptr.numel() - 1, col_ind.numel()
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((n_src, dim), device="cuda", generator=gen)
    w = torch.rand((E,), device="cuda", generator=gen) + 0.5
    G = torch.randn((n_dst, 2 * dim), device="cuda", generator=gen)

    def leaves(want_x, want_w):
        return x.clone().requires_grad_(want_x), w.clone().requires_grad_(want_w)

    def bwd_of(out, *ls):
        def f():
            for l in ls:
                l.grad = None
            torch.autograd.backward(out, G, retain_graph=True)
        return f

    # ---- the weighted op
    xw, ww = leaves(True, True)
    fwd = base.timed_all(lambda: agg_concat_weighted(xw, row_ptr, col_ind, ww, "mean"), warmup, reps)
    out_xw = agg_concat_weighted(xw, row_ptr, col_ind, ww, "mean")
    bwd_xw_f = bwd_of(out_xw, xw, ww)
    bwd_xw = base.timed_all(bwd_xw_f, warmup, reps)
    split = kernel_ms(bwd_xw_f, max(3, reps // 2)) if split_kernels else None
    x1, w1 = leaves(True, False)
    bwd_x = base.timed_all(bwd_of(agg_concat_weighted(x1, row_ptr, col_ind, w1, "mean"), x1), warmup, reps)
    x2, w2 = leaves(False, True)
    bwd_w = base.timed_all(bwd_of(agg_concat_weighted(x2, row_ptr, col_ind, w2, "mean"), w2), warmup, reps)

    # ---- unweighted agg_concat, same process, same block
    xu = x.clone().requires_grad_(True)
    u_fwd = base.timed_all(lambda: agg_concat(xu, row_ptr, col_ind, "mean"), warmup, reps)
    u_bwd = base.timed_all(bwd_of(agg_concat(xu, row_ptr, col_ind, "mean"), xu), warmup, reps)

    # ---- the torch composite, forward and backward through autograd
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device="cuda"), deg)
    col64 = col_ind.long()
    rdeg = (1.0 / deg.clamp(min=1).float())[:, None]

    def composite(x_, w_):
        agg = torch.zeros((n_dst, dim), device="cuda").index_add_(0, dst, x_[col64] * w_[:, None])
        return torch.cat([agg * rdeg, x_[:n_dst]], dim=1)
    xc, wc = leaves(True, True)
    c_fwd = base.timed_all(lambda: composite(xc, wc), warmup, reps)
    c_bwd_xw = base.timed_all(bwd_of(composite(xc, wc), xc, wc), warmup, reps)
    xc1, wc1 = leaves(True, False)
    c_bwd_x = base.timed_all(bwd_of(composite(xc1, wc1), xc1), warmup, reps)

    # the same op within rounding (norm-wise: the composite adds a hub's terms in whatever order its atomics land)
    def rel(a_, b_):
        return float((a_ - b_).norm() / b_.norm().clamp(min=1e-30))
    bwd_xw_f()
    bwd_of(composite(xc, wc), xc, wc)()
    assert rel(out_xw, composite(xc, wc)) < 1e-5
    assert rel(xw.grad, xc.grad) < 1e-5 and rel(ww.grad, wc.grad) < 1e-5

    F = dim
    fwd_bytes = E * (8 + 4 * F) + n_dst * (4 + 12 * F)
    u_fwd_bytes = E * (4 + 4 * F) + n_dst * (4 + 12 * F)
    fold_bytes = E * (12 + 4 * F) + n_src * 4 * F + n_dst * 4 * F
    u_fold_bytes = E * (8 + 4 * F) + n_src * 4 * F + n_dst * 4 * F
    weight_bytes = E * (12 + 4 * F) + n_dst * 4 * F
    med = lambda ms: statistics.median(ms)
    spread_f, spread_b = max(u_fwd) / med(u_fwd), max(u_bwd) / med(u_bwd)
    allow_f = fwd_bytes / u_fwd_bytes * spread_f
    allow_b = fold_bytes / u_fold_bytes * spread_b
    counts = torch.bincount(col64, minlength=n_src)
    res = {"shape": name, "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": dim,
           "max_edges_per_source": int(counts.max()),
           "forward_ms": stats(fwd), "backward_x_ms": stats(bwd_x), "backward_xw_ms": stats(bwd_xw),
           "backward_w_ms": stats(bwd_w),
           "forward_frac_8TBps": round(fwd_bytes / med(fwd) / 1e-3 / PEAK, 4),
           "agg_concat_forward_ms": stats(u_fwd), "agg_concat_backward_ms": stats(u_bwd),
           "agg_concat_forward_frac_8TBps": round(u_fwd_bytes / med(u_fwd) / 1e-3 / PEAK, 4),
           "torch_forward_ms": stats(c_fwd), "torch_backward_x_ms": stats(c_bwd_x), "torch_backward_xw_ms": stats(c_bwd_xw),
           "speedup_forward_vs_torch": round(med(c_fwd) / med(fwd), 2),
           "speedup_backward_x_vs_torch": round(med(c_bwd_x) / med(bwd_x), 2),
           "speedup_backward_xw_vs_torch": round(med(c_bwd_xw) / med(bwd_xw), 2),
           "gate_faster_than_torch": bool(med(fwd) < med(c_fwd) and med(bwd_x) < med(c_bwd_x) and
                                          med(bwd_xw) < med(c_bwd_xw)),
           "forward_over_agg_concat": round(med(fwd) / med(u_fwd), 4), "forward_allowed": round(allow_f, 4),
           "backward_x_over_agg_concat": round(med(bwd_x) / med(u_bwd), 4), "backward_x_allowed": round(allow_b, 4),
           "gate_forward_within_byte_ratio": bool(med(fwd) / med(u_fwd) <= allow_f),
           "gate_backward_x_within_byte_ratio": bool(med(bwd_x) / med(u_bwd) <= allow_b)}
    if split is not None:
        fold_ms, weight_ms = split
        res.update({"fold_ms": round(fold_ms, 4), "fold_frac_8TBps": round(fold_bytes / fold_ms / 1e-3 / PEAK, 4),
                    "weight_kernel_ms": round(weight_ms, 4),
                    "weight_kernel_frac_8TBps": round(weight_bytes / weight_ms / 1e-3 / PEAK, 4)})
    else:
        res.update({"fold_ms": None, "fold_frac_8TBps": None, "weight_kernel_ms": None, "weight_kernel_frac_8TBps": None})
    torch.cuda.empty_cache()
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--dim", type=int, default=128)
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
    assert torch.cuda.is_available(), "bench_weighted_agg.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges

    results = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    E = a.n_dst * a.fanout
    for shape in a.shapes.split(","):
        if shape == "a":
            col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
            results.append(run_shape("a_uniform", row_ptr, col, a.n_src, a.dim, a.warmup, a.reps, not a.no_kernel_split))
        elif shape == "b":
            col = base.powerlaw_ids(a.n_src, E, 0.8, gen)
            results.append(run_shape("b_powerlaw", row_ptr, col, a.n_src, a.dim, a.warmup, a.reps, not a.no_kernel_split))
        elif shape == "c":
            rp, ci, n_src = base.c5_layer0(wgth, comm, a.nodes, 29, 1024, [30, 30])
            results.append(run_shape("c_c5_layer0", rp, ci, n_src, a.dim, a.warmup, a.reps, not a.no_kernel_split))
    line = {"bench": "weighted_agg", "chunk_edges": chunk_edges(), "peak_Bps": PEAK, "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
