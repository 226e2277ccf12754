#!/usr/bin/env python3
"""Timing of LABOR layer-neighbour sampling (wholegraph_amd/torch/wholegraph_ops.py: labor_sample -> csrc/kernels/labor.hip) on
one MI355X, and what it is for: the distinct nodes a sampled hop touches. Writes ONE JSON line into profiles/labor_bench.json
(and prints it).

Graphs (`--col-dists`, one after the other in one process): the papers100M-shaped graph of the other sampler benches (`--nodes`
nodes, degrees uniform in [0, 58], CHUNKED, int32 ids) with column ids drawn uniformly ("uniform") and from the truncated power
law of scripts/bench_walk.py ("powerlaw": hub nodes that many rows share). Centres: the node sets of
scripts/bench_temporal_sample.py. Per graph and set, in one process, alternating, at fan-out `--fanout`:
  fixed, poisson   labor_sample in either mode
  plain            unweighted_sample_without_replacement, the existing sampler: the yardstick
each the median of `--reps` calls after `--warmup`, the three called in turn, timed with events, every call with a seed of its
own. Then a 2-hop [fanout, fanout] sample from `--seeds` seed nodes by the three samplers, hop by hop with append_unique (LABOR
with one seed for both hops), and per hop the sampled entries and the distinct nodes after append_unique: the size of the next
hop's batch and of the feature gather.

The measurement runs in a child process under `timeout` (--step-timeout seconds); the parent never opens the GPU."""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SETS = ((3_000, 2), (20_000, 4), (100_000, 4))      # (roots, steps)


def alternating(fns, warmup, reps):
    """-> {name: median ms of one call}, the functions called in turn, round after round, each call between two events"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: statistics.median(v) for name, v in ms.items()}


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_labor.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding            # (first: the helper scripts below put the repository in front of the path)
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch import graph_ops
    from bench_walk import build_graph
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    graphs = {}
    for dist in a.col_dists.split(","):
        wrow, wcol, wwgt, edges = build_graph(wgth, comm, a.nodes, 29)      # (power-law column ids)
        wgth.destroy_wholememory_tensor(wwgt)
        if dist == "uniform":
            lcol, gen = wcol.get_local_tensor()[0], torch.Generator(device="cuda").manual_seed(100)
            for s0 in range(0, edges, 1 << 28):
                e0 = min(edges, s0 + (1 << 28))
                lcol[s0:e0] = torch.randint(0, a.nodes, (e0 - s0,), device="cuda", generator=gen, dtype=torch.int32)
        row, col, seeds = wrow.wmb_tensor, wcol.wmb_tensor, itertools.count(1000)
        samplers = {"fixed": lambda c, s: wops.labor_sample(row, col, c, a.fanout, s, "fixed"),
                    "poisson": lambda c, s: wops.labor_sample(row, col, c, a.fanout, s, "poisson"),
                    "plain": lambda c, s: wops.unweighted_sample_without_replacement(row, col, c, a.fanout, s)}
        gen = torch.Generator(device="cuda").manual_seed(7)
        sets = {}
        for roots, steps in SETS:
            starts = torch.randint(0, a.nodes, (roots,), device="cuda", generator=gen, dtype=torch.int32)
            walks = wops.random_walk(row, col, starts, steps, 3)
            centres = torch.unique(walks[walks >= 0])
            res = {"centres": int(centres.shape[0])}
            for name, fn in samplers.items():
                res[name + "_entries"] = int(fn(centres, 5)[0][-1])
            ms = alternating({name: (lambda fn=fn: fn(centres, next(seeds))) for name, fn in samplers.items()}, a.warmup, a.reps)
            res.update({name + "_ms": round(v, 4) for name, v in ms.items()})
            for name in ("fixed", "poisson"):
                res[name + "_over_plain"] = round(res[name + "_ms"] / res["plain_ms"], 2)
            sets["%dx%d" % (roots, steps)] = res
        batch = torch.randint(0, a.nodes, (a.seeds,), device="cuda", generator=gen, dtype=torch.int32)
        hops = {}
        for name, fn in samplers.items():
            frontier, per_hop = batch, []
            for depth in range(2):      # LABOR: one seed for both hops (layer_dependency); plain: one per hop
                _, neighbours = fn(frontier, 77 if name != "plain" else 77 + depth)
                widened = graph_ops.append_unique(frontier, neighbours)
                per_hop.append({"centres": int(frontier.shape[0]), "entries": int(neighbours.shape[0]),
                                "distinct_after_append_unique": int(widened.shape[0])})
                frontier = widened
            hops[name] = per_hop
        for name in ("fixed", "poisson"):
            hops["plain_over_" + name] = [round(p["distinct_after_append_unique"] / q["distinct_after_append_unique"], 3)
                                          for p, q in zip(hops["plain"], hops[name])]
        graphs[dist] = {"edges": edges, "mean_degree": round(edges / a.nodes, 2), "sets": sets, "two_hops": hops}
        wgth.destroy_wholememory_tensor(wrow)
        wgth.destroy_wholememory_tensor(wcol)
        torch.cuda.empty_cache()
    line = {"bench": "labor", "library": os.path.relpath(binding.LIB_PATH, ROOT), "graph_nodes": a.nodes, "fanout": a.fanout,
            "seeds": a.seeds, "warmup": a.warmup, "reps": a.reps, "graphs": graphs}
    print("LABOR_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--fanout", type=int, default=30)
    p.add_argument("--seeds", type=int, default=1024, help="seed nodes of the 2-hop sample")
    p.add_argument("--col-dists", default="uniform,powerlaw", help="comma-separated: uniform, powerlaw")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "labor_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child"]
    for name in ("warmup", "reps", "nodes", "fanout", "seeds", "col_dists"):
        cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("LABOR_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_labor: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return 1
    text = lines[-1][len("LABOR_BENCH "):]
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
