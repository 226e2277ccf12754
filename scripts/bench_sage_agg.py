#!/usr/bin/env python3
"""Timing of the GraphSAGE neighbour aggregation (wholegraph_amd/torch/aggregation.py -> csrc/kernels/agg.hip) on one
MI355X; prints ONE JSON line.

Shapes:
  a  uniform:   n_dst 333,334 targets x fan-out 30 (E = 10 M), n_src 2 M, F 128 (x = 1 GB, past the 256 MiB Infinity Cache)
  b  power-law: the same with col_ind drawn from a truncated power law (bench.py --col-dist powerlaw, s 0.8): hub sources
     with thousands of edges
  c  layer 0 (the outermost block) of a BASELINE config 5 sample: 1024 seeds, fan-outs 30,30, on a graph built the way
     bench.py --op sample_gather builds it (degrees uniform in [0, 2 x 29], power-law neighbour ids)

Per shape: the forward, the full backward, and the backward split into the edge index (the id sort of col_ind + the
target / run lookups of agg_bwd_prep_kernel) and the fold (agg_bwd_chunk_kernel + agg_bwd_fold_kernel) from per-kernel
device times (torch.profiler). Algorithmic bytes: forward E(4 + 4F) + n_dst(4 + 12F); fold E(8 + 4F) + n_src 4F + n_dst 4F;
the fraction is of 8 TB/s. The torch composite of the same op in the same process (index_select + index_add_ segment sum
+ cat for the forward; index_select + index_add_ for the backward) gives the ratios.

--dtype float16 | bfloat16 times the op on 16-bit rows (csrc/kernels/agg_half.hip; bytes with 2-byte rows: forward
E(4 + 2F) + n_dst(4 + 6F); fold E(8 + 2F) + n_src 2F + n_dst 2F) and, on the same block in the same process, the two
baselines it is judged against: the fp32 op on x.float() (with the min and max of its repetitions, its run-to-run spread)
and the "cast composite" a user had to write without 16-bit rows, agg_concat(x.float(), ...).to(T), forward and backward
through autograd. The 16-bit result is also checked bit for bit against the fp32 result rounded once."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


def timed_all(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def timed(fn, warmup, reps):
    return statistics.median(timed_all(fn, warmup, reps))


def kernel_split(fn, reps):
    """mean device ms per call of (edge index, fold) kernels, from torch.profiler's kernel records; None when the profiler
    records no kernel of this library"""
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
    fold = index = 0.0
    seen = False
    for ev in prof.events():
        name = ev.name
        t = getattr(ev, "device_time", None)
        if t is None:
            t = getattr(ev, "cuda_time", 0.0)
        if ev.device_type != torch.autograd.DeviceType.CUDA:
            continue
        if "agg_bwd_chunk_kernel" in name or "agg_bwd_fold_kernel" in name or "agg16_bwd_" in name:
            fold += t
            seen = True
        elif "agg_forward_kernel" not in name and "agg16_forward_kernel" not in name and "elementwise" not in name.lower() and "fill" not in name.lower():
            index += t   # the id sort's kernels and agg_bwd_prep_kernel
    if not seen:
        return None
    return index / 1000.0 / reps, fold / 1000.0 / reps


def powerlaw_ids(n, count, s, gen):
    import torch
    u = torch.rand(count, device="cuda", generator=gen, dtype=torch.float64)
    rank_k = (u.pow_(1.0 / (1.0 - s)) * n).to(torch.int64).clamp_(0, n - 1)
    return ((rank_k * 2654435761) % n).to(torch.int32)


def c5_layer0(wgth, comm, nodes, avg, seeds_n, fanouts):
    """layer 0 of one sample on the bench.py sample_gather graph (CHUNKED, one GPU)"""
    import torch
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
    out = rp[0].clone(), ci[0].clone(), int(tg[0].numel())
    del g, lcol
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
    torch.cuda.synchronize()
    return out


def run_shape(name, row_ptr, col_ind, n_src, dim, warmup, reps, split_kernels=True):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    n_dst, E = row_ptr.numel() - 1, col_ind.numel()
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((n_src, dim), device="cuda", generator=gen).requires_grad_(True)
    out = agg_concat(x, row_ptr, col_ind, "mean")
    G = torch.randn(tuple(out.shape), device="cuda", generator=gen)

    fwd_ms = timed(lambda: agg_concat(x, row_ptr, col_ind, "mean"), warmup, reps)

    def bwd():
        x.grad = None
        torch.autograd.backward(out, G, retain_graph=True)
    bwd_ms = timed(bwd, warmup, reps)
    split = kernel_split(bwd, max(3, reps // 2)) if split_kernels else None

    # torch composite, same process
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device="cuda"), deg)
    col64 = col_ind.long()
    rdeg = (1.0 / deg.clamp(min=1).float())[:, None]
    xd = x.detach()

    def comp_fwd():
        agg = torch.zeros((n_dst, dim), device="cuda").index_add_(0, dst, xd.index_select(0, col64))
        return torch.cat([agg * rdeg, xd[:n_dst]], dim=1)

    def comp_bwd():
        t = (G[:, :dim] * rdeg).index_select(0, dst)
        gx = torch.zeros((n_src, dim), device="cuda").index_add_(0, col64, t)
        gx[:n_dst] += G[:, dim:]
        return gx
    cf_ms = timed(comp_fwd, warmup, reps)
    cb_ms = timed(comp_bwd, warmup, reps)
    # same op within rounding (norm-wise: the composite adds a hub's terms in whatever order its atomics land)
    def rel(a_, b_):
        return float((a_ - b_).norm() / b_.norm().clamp(min=1e-30))
    assert rel(out, comp_fwd()) < 1e-5
    bwd()
    assert rel(x.grad, comp_bwd()) < 1e-5

    fwd_bytes = E * (4 + 4 * dim) + n_dst * (4 + 12 * dim)
    fold_bytes = E * (8 + 4 * dim) + n_src * 4 * dim + n_dst * 4 * dim
    counts = torch.bincount(col_ind.long(), minlength=n_src)
    res = {"shape": name, "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": dim,
           "max_edges_per_source": int(counts.max()), "median_edges_per_used_source": float(counts[counts > 0].median()),
           "forward_ms": round(fwd_ms, 4), "forward_GBps": round(fwd_bytes / fwd_ms / 1e6, 1),
           "forward_frac_8TBps": round(fwd_bytes / fwd_ms / 1e-3 / PEAK, 4),
           "backward_ms": round(bwd_ms, 4),
           "torch_forward_ms": round(cf_ms, 4), "torch_backward_ms": round(cb_ms, 4),
           "speedup_forward_vs_torch": round(cf_ms / fwd_ms, 2), "speedup_backward_vs_torch": round(cb_ms / bwd_ms, 2)}
    if split is not None:
        index_ms, fold_ms = split
        res.update({"index_ms": round(index_ms, 4), "fold_ms": round(fold_ms, 4),
                    "fold_GBps": round(fold_bytes / fold_ms / 1e6, 1),
                    "fold_frac_8TBps": round(fold_bytes / fold_ms / 1e-3 / PEAK, 4)})
    else:
        res.update({"index_ms": None, "fold_ms": None, "fold_GBps": None, "fold_frac_8TBps": None})
    del x, out, G
    torch.cuda.empty_cache()
    return res


def run_shape_16(name, row_ptr, col_ind, n_src, dim, warmup, reps, dtype, split_kernels=True):
    """the op on rows of `dtype` (fp16 / bf16), the fp32 op and the cast composite on the same block"""
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    n_dst, E = row_ptr.numel() - 1, col_ind.numel()
    gen = torch.Generator(device="cuda").manual_seed(3)
    x16 = torch.randn((n_src, dim), device="cuda", generator=gen).to(dtype).requires_grad_(True)
    out16 = agg_concat(x16, row_ptr, col_ind, "mean")
    G16 = torch.randn(tuple(out16.shape), device="cuda", generator=gen).to(dtype)
    x32 = x16.detach().float().requires_grad_(True)
    out32 = agg_concat(x32, row_ptr, col_ind, "mean")
    G32 = G16.float()
    xc = x16.detach().clone().requires_grad_(True)   # the cast composite's leaf
    outc = agg_concat(xc.float(), row_ptr, col_ind, "mean").to(dtype)

    def bwd_of(x, out, G):
        def f():
            x.grad = None
            torch.autograd.backward(out, G, retain_graph=True)
        return f
    bwd16, bwd32, bwdc = bwd_of(x16, out16, G16), bwd_of(x32, out32, G32), bwd_of(xc, outc, G16)
    # the same op: the 16-bit result is the fp32 result rounded once, bit for bit (and so is the cast composite's)
    bwd16(), bwd32(), bwdc()
    assert torch.equal(out16.view(torch.int16), out32.to(dtype).view(torch.int16))
    assert torch.equal(x16.grad.view(torch.int16), x32.grad.to(dtype).view(torch.int16))
    assert torch.equal(xc.grad.view(torch.int16), x16.grad.view(torch.int16))

    def stats(ms):
        return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)
    fwd = stats(timed_all(lambda: agg_concat(x16, row_ptr, col_ind, "mean"), warmup, reps))
    bwd = stats(timed_all(bwd16, warmup, reps))
    split = kernel_split(bwd16, max(3, reps // 2)) if split_kernels else None
    f32_fwd = stats(timed_all(lambda: agg_concat(x32, row_ptr, col_ind, "mean"), warmup, reps))
    f32_bwd = stats(timed_all(bwd32, warmup, reps))
    f32_split = kernel_split(bwd32, max(3, reps // 2)) if split_kernels else None
    xd = x16.detach()
    cast_fwd = stats(timed_all(lambda: agg_concat(xd.float(), row_ptr, col_ind, "mean").to(dtype), warmup, reps))
    cast_bwd = stats(timed_all(bwdc, warmup, reps))

    fwd_bytes = E * (4 + 2 * dim) + n_dst * (4 + 6 * dim)
    fold_bytes = E * (8 + 2 * dim) + n_src * 2 * dim + n_dst * 2 * dim
    counts = torch.bincount(col_ind.long(), minlength=n_src)
    res = {"shape": name, "dtype": str(dtype).replace("torch.", ""), "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": dim,
           "max_edges_per_source": int(counts.max()), "median_edges_per_used_source": float(counts[counts > 0].median()),
           "forward_ms": fwd[0], "forward_ms_min_max": fwd[1:], "forward_GBps": round(fwd_bytes / fwd[0] / 1e6, 1),
           "forward_frac_8TBps": round(fwd_bytes / fwd[0] / 1e-3 / PEAK, 4),
           "backward_ms": bwd[0], "backward_ms_min_max": bwd[1:],
           "fp32_forward_ms": f32_fwd[0], "fp32_forward_ms_min_max": f32_fwd[1:],
           "fp32_backward_ms": f32_bwd[0], "fp32_backward_ms_min_max": f32_bwd[1:],
           "cast_forward_ms": cast_fwd[0], "cast_forward_ms_min_max": cast_fwd[1:],
           "cast_backward_ms": cast_bwd[0], "cast_backward_ms_min_max": cast_bwd[1:],
           "forward_over_fp32": round(fwd[0] / f32_fwd[0], 3), "backward_over_fp32": round(bwd[0] / f32_bwd[0], 3),
           "forward_over_cast": round(fwd[0] / cast_fwd[0], 3), "backward_over_cast": round(bwd[0] / cast_bwd[0], 3),
           # the gates: faster than the cast composite; not slower than the fp32 op by more than that op's own spread
           "faster_than_cast": bool(fwd[0] < cast_fwd[0] and bwd[0] < cast_bwd[0]),
           "within_fp32_spread": bool(fwd[0] <= f32_fwd[0] + (f32_fwd[2] - f32_fwd[1]) and
                                      bwd[0] <= f32_bwd[0] + (f32_bwd[2] - f32_bwd[1]))}
    if split is not None:
        index_ms, fold_ms = split
        res.update({"index_ms": round(index_ms, 4), "fold_ms": round(fold_ms, 4),
                    "fold_GBps": round(fold_bytes / fold_ms / 1e6, 1),
                    "fold_frac_8TBps": round(fold_bytes / fold_ms / 1e-3 / PEAK, 4)})
        if f32_split is not None:
            res.update({"fp32_index_ms": round(f32_split[0], 4), "fp32_fold_ms": round(f32_split[1], 4),
                        "fold_over_fp32": round(fold_ms / f32_split[1], 3)})
    else:
        res.update({"index_ms": None, "fold_ms": None, "fold_GBps": None, "fold_frac_8TBps": None})
    del x16, out16, G16, x32, out32, G32, xc, outc, xd
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
    p.add_argument("--dtype", choices=("float32", "float16", "bfloat16"), default="float32",
                   help="row type; a 16-bit type also times the fp32 op and the cast composite on the same block")
    p.add_argument("--out", help="also write the JSON line to this file")
    p.add_argument("--no-kernel-split", action="store_true",
                   help="skip the torch.profiler split of the backward (when an outer profiler such as rocprofv3 traces the run)")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_sage_agg.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    from wholegraph_amd.torch.aggregation import chunk_edges

    if a.dtype == "float32":
        run = run_shape
    else:
        def run(*args):
            return run_shape_16(*args[:7], getattr(torch, a.dtype), args[7])
    results = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    row_ptr = (torch.arange(a.n_dst + 1, device="cuda", dtype=torch.int32) * a.fanout)
    E = a.n_dst * a.fanout
    for shape in a.shapes.split(","):
        if shape == "a":
            col = torch.randint(0, a.n_src, (E,), device="cuda", generator=gen, dtype=torch.int32)
            results.append(run("a_uniform", row_ptr, col, a.n_src, a.dim, a.warmup, a.reps, not a.no_kernel_split))
        elif shape == "b":
            col = powerlaw_ids(a.n_src, E, 0.8, gen)
            results.append(run("b_powerlaw", row_ptr, col, a.n_src, a.dim, a.warmup, a.reps, not a.no_kernel_split))
        elif shape == "c":
            rp, ci, n_src = c5_layer0(wgth, comm, a.nodes, 29, 1024, [30, 30])
            results.append(run("c_c5_layer0", rp, ci, n_src, a.dim, a.warmup, a.reps, not a.no_kernel_split))
    line = {"bench": "sage_agg", "chunk_edges": chunk_edges(), "peak_Bps": PEAK, "results": results}
    if a.dtype != "float32":
        line["dtype"] = a.dtype
    by = {r["shape"]: r for r in results}
    if "a_uniform" in by and "b_powerlaw" in by and by["a_uniform"]["fold_ms"] and by["b_powerlaw"]["fold_ms"]:
        # at equal bytes: both shapes move the same algorithmic fold bytes (same E, n_src, n_dst, F)
        line["fold_powerlaw_over_uniform"] = round(by["b_powerlaw"]["fold_ms"] / by["a_uniform"]["fold_ms"], 3)
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
