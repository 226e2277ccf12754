#!/usr/bin/env python3
"""Timing of the multi-aggregator neighbour aggregation (wholegraph_amd/torch/pna_aggregation.py -> csrc/kernels/pna.hip)
on one MI355X; writes ONE JSON line into profiles/pna_bench.json (and prints it).

Block: layer 0 of a BASELINE config 5 sample (1024 seeds, fan-outs 30,30; scripts/bench_sage_agg.py's c5_layer0), rows of
`--dim` fp32 columns. In one process, on that block, forward and forward + backward of
  pna_all    agg_concat_pna with all five aggregators
  pna_max    agg_concat_pna with ["max"] alone (GraphSAGE-max)
  agg_mean   agg_concat(..., "mean")
  torch_all  the torch composite of all five: index_select, index_add_ and scatter_reduce (amin / amax), autograd backward
The variants alternate: `--rounds` rounds, in each the median of `--reps` calls of every variant after `--warmup`; the result
is the median over the rounds, with the lowest and highest round next to it (the run-to-run spread inside the process). The
ratios are formed round by round. Algorithmic bytes of a forward with A aggregators: E (4 + 4 dim) (col_ind, a neighbour
row) + n_dst 4 dim (the own row) + n_dst 4 (A + 1) dim (out); with fan-out 30 the all-five forward moves
(30 + 1 + 6) / (30 + 1 + 2) = 1.12 times the bytes of agg_concat's.

The measurement runs in a child process under `timeout` (--step-timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ALL = ("sum", "mean", "min", "max", "std")


def composite(x, row_ptr, col, dst, n):
    """all five aggregators and the own row, in plain torch"""
    import torch
    n_dst, F = row_ptr.numel() - 1, x.shape[1]
    xe = x.index_select(0, col)
    zero = torch.zeros((n_dst, F), device=x.device, dtype=x.dtype)
    idx = dst[:, None].expand(-1, F)
    S = zero.index_add(0, dst, xe)
    mean = S / n
    mn = zero.scatter_reduce(0, idx, xe, "amin", include_self=False)
    mx = zero.scatter_reduce(0, idx, xe, "amax", include_self=False)
    var = zero.index_add(0, dst, xe * xe) / n - mean * mean
    std = (var.relu() + 1e-5).sqrt()
    return torch.cat([S, mean, mn, mx, std, x[:n_dst]], dim=1)


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_pna.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from bench_sage_agg import PEAK, c5_layer0, timed
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    row_ptr, col_ind, n_src = c5_layer0(wgth, comm, a.nodes, 29, 1024, [30, 30])
    n_dst, E, F = row_ptr.numel() - 1, col_ind.numel(), a.dim
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((n_src, F), device="cuda", generator=gen)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device="cuda"), deg)
    col64 = col_ind.long()
    n = deg.clamp(min=1).float()[:, None]
    ops = {
        "pna_all": (lambda t: agg_concat_pna(t, row_ptr, col_ind, ALL), 6),
        "pna_max": (lambda t: agg_concat_pna(t, row_ptr, col_ind, ["max"]), 2),
        "agg_mean": (lambda t: agg_concat(t, row_ptr, col_ind, "mean"), 2),
        "torch_all": (lambda t: composite(t, row_ptr, col64, dst, n), 6),
    }
    steps = {}
    for name, (fn, slots) in ops.items():
        G = torch.randn((n_dst, slots * F), device="cuda", generator=gen)
        xg = x.clone().requires_grad_(True)

        def fwd(fn=fn):
            with torch.no_grad():
                fn(x)

        def both(fn=fn, xg=xg, G=G):
            xg.grad = None
            fn(xg).backward(G)
        steps[name + "_forward"] = fwd
        steps[name + "_forward_backward"] = both
    # the op against the composite, on this block, before anything is timed
    got, want = ops["pna_all"][0](x), ops["torch_all"][0](x)
    live = (deg > 0)[:, None].float()
    rel = float(((got - want) * live).norm() / (want * live).norm())
    assert rel < 1e-5, rel
    rounds = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            rounds[k].append(timed(fn, a.warmup, a.reps))
    res = {}
    for k, ms in rounds.items():
        res[k + "_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

    def ratio(num, den):
        r = [p / q for p, q in zip(rounds[num], rounds[den])]
        return {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3)}
    fwd_bytes = lambda A: E * (4 + 4 * F) + n_dst * 4 * F + n_dst * 4 * (A + 1) * F
    res["ratios"] = {
        "pna_all_forward_over_agg_mean_forward": ratio("pna_all_forward", "agg_mean_forward"),
        "byte_count_expectation": round(fwd_bytes(5) / fwd_bytes(1), 3),
        "pna_all_forward_over_torch": ratio("pna_all_forward", "torch_all_forward"),
        "pna_all_forward_backward_over_torch": ratio("pna_all_forward_backward", "torch_all_forward_backward"),
        "pna_all_forward_backward_over_agg_mean": ratio("pna_all_forward_backward", "agg_mean_forward_backward"),
        "pna_max_forward_over_agg_mean_forward": ratio("pna_max_forward", "agg_mean_forward"),
    }
    fwd_ms = res["pna_all_forward_ms"]["median"]
    line = {"bench": "pna", "block": "c5_layer0", "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": F,
            "mean_degree": round(E / max(n_dst, 1), 2), "warmup": a.warmup, "reps": a.reps, "rounds": a.rounds,
            "peak_Bps": PEAK, "pna_all_forward_GBps": round(fwd_bytes(5) / fwd_ms / 1e6, 1),
            "pna_all_forward_frac_8TBps": round(fwd_bytes(5) / fwd_ms / 1e-3 / PEAK, 4), **res}
    print("PNA_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--step-timeout", type=int, default=420, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pna_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--rounds", str(a.rounds), "--dim", str(a.dim), "--nodes", str(a.nodes)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("PNA_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_pna: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return child.returncode or 1
    line = lines[-1][len("PNA_BENCH "):]
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
