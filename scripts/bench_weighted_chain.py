#!/usr/bin/env python3
"""Timing of WEIGHTED multi-layer neighbour sampling (GraphStructure.multilayer_sample_without_replacement(weight_name=...))
on one MI355X; prints ONE JSON line and writes it to --out.

Graph: the synthetic graph of bench.py --op sample_gather (BASELINE config 5: 111 M nodes, degrees uniform in [0, 2 x 29],
int32 neighbour ids, CHUNKED), built once per --col-dist setting (uniform, powerlaw with exponent 0.8), plus one float
weight per edge, 10^U(-3, 3) from a seeded generator. Batch: 1024 seeds, fan-outs 30,30, fixed per-hop sampler seeds.
One step = the sample call + a device synchronise (no feature gather: the sampler is what is compared). Per graph:
  weighted     the call with weight_name="w" as the imported package routes it (this tree: the one-call chain on
               sample_weighted_small_kernel; a package without the weighted chain: sampler + append_unique per hop)
  unweighted   the same call without weights, the floor
Median, min and max of --steps timed steps after --warmup warm-up steps, and a checksum of the weighted sample.

--package-root DIR imports wholegraph_amd from DIR instead of this tree (a build of another commit, e.g. what
scripts/build_variant.sh leaves under experiments/variants/NAME); --parent-json FILE embeds the line such a run wrote, with
the speed-up over it and whether both produced the same sample."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def powerlaw_ids(n, count, s, gen):
    import torch
    u = torch.rand(count, device="cuda", generator=gen, dtype=torch.float64)
    rank_k = (u.pow_(1.0 / (1.0 - s)) * n).to(torch.int64).clamp_(0, n - 1)
    return ((rank_k * 2654435761) % n).to(torch.int32)


def timed_steps(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=111_059_956)
    p.add_argument("--avg-degree", type=int, default=29)
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanouts", default="30,30")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--col-dists", default="uniform,powerlaw")
    p.add_argument("--package-root", default=ROOT)
    p.add_argument("--parent-json", default=None)
    p.add_argument("--label", default="tree")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_chain_bench.json"))
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    fanouts = [int(x) for x in a.fanouts.split(",")]
    hop_seeds = [1000 + 17 * i for i in range(len(fanouts))]
    nodes, avg = a.nodes, a.avg_degree

    gen = torch.Generator(device="cuda").manual_seed(1)
    row = torch.zeros(nodes + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(torch.randint(0, 2 * avg + 1, (nodes,), device="cuda", generator=gen), 0, out=row[1:])
    edges = int(row[-1])
    wrow = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [nodes + 1], torch.int64, [1])
    wcol = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [edges], torch.int32, [1])
    wwgt = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [edges], torch.float32, [1])
    wrow.get_local_tensor()[0].copy_(row)
    del row
    lcol, lwgt = wcol.get_local_tensor()[0], wwgt.get_local_tensor()[0]
    genw = torch.Generator(device="cuda").manual_seed(4242)
    for s0 in range(0, edges, 1 << 28):
        e0 = min(edges, s0 + (1 << 28))
        lwgt[s0:e0] = torch.pow(10.0, torch.rand(e0 - s0, device="cuda", generator=genw) * 6.0 - 3.0)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    g.set_edge_attribute("w", wwgt)
    has_chain = "wholememory_ext_multilayer_sample_weighted" in binding.PROTOTYPES

    graphs = {}
    for dist in a.col_dists.split(","):
        gen2 = torch.Generator(device="cuda").manual_seed(100)
        for s0 in range(0, edges, 1 << 28):
            e0 = min(edges, s0 + (1 << 28))
            if dist == "powerlaw":
                lcol[s0:e0] = powerlaw_ids(nodes, e0 - s0, 0.8, gen2)
            else:
                lcol[s0:e0] = torch.randint(0, nodes, (e0 - s0,), device="cuda", generator=gen2, dtype=torch.int32)
        seeds = torch.randint(0, nodes, (a.seeds,), device="cuda", generator=gen2, dtype=torch.int32)
        torch.cuda.synchronize()
        weighted = lambda: g.multilayer_sample_without_replacement(seeds, fanouts, weight_name="w", random_seeds=hop_seeds)
        plain = lambda: g.multilayer_sample_without_replacement(seeds, fanouts, random_seeds=hop_seeds)
        tg, ei, rp, ci = weighted()
        torch.cuda.synchronize()
        r = {"frontier_sizes": [int(t.numel()) for t in tg], "sampled_edges": sum(int(c.numel()) for c in ci),
             "checksum": [int(t.long().sum().item()) for t in tg] + [int(c.long().sum().item()) for c in ci]}
        del tg, ei, rp, ci
        r["weighted"] = timed_steps(weighted, a.warmup, a.steps)
        r["unweighted"] = timed_steps(plain, a.warmup, a.steps)
        r["weighted_over_unweighted"] = round(r["weighted"]["median_ms"] / r["unweighted"]["median_ms"], 2)
        graphs[dist] = r

    res = {"bench": "weighted_chain", "label": a.label, "weighted_route": "one-call chain" if has_chain else "hop by hop, two ops per hop",
           "nodes": nodes, "edges": edges, "seeds": a.seeds, "fanouts": fanouts, "steps": a.steps, "warmup": a.warmup,
           "timing": "host clock around the sample call + device synchronise, ms per step", "graphs": graphs}
    if a.parent_json and os.path.exists(a.parent_json):
        parent = json.loads(open(a.parent_json).read().strip().splitlines()[-1])
        res["parent"] = {"label": parent["label"], "weighted_route": parent["weighted_route"], "graphs": parent["graphs"]}
        for dist, r in graphs.items():
            pr = parent["graphs"].get(dist)
            if pr is None:
                continue
            r["same_sample_as_parent"] = pr["checksum"] == r["checksum"] and pr["frontier_sizes"] == r["frontier_sizes"]
            r["speedup_over_parent"] = round(pr["weighted"]["median_ms"] / r["weighted"]["median_ms"], 2)
            # the parent's own run-to-run spread is cleared when this tree's slowest step beats the parent's fastest
            r["clears_parent_spread"] = r["weighted"]["max_ms"] < pr["weighted"]["min_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    for t in (wrow, wcol, wwgt):
        wgth.destroy_wholememory_tensor(t)


if __name__ == "__main__":
    main()
