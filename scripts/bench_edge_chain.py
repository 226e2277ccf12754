#!/usr/bin/env python3
"""Timing of multi-layer neighbour sampling WITH the attributes of the sampled edges
(GraphStructure.multilayer_sample_with_edge_attributes) on one MI355X; prints ONE JSON line and writes it to --out.

Graph: the synthetic graph of bench.py --op sample_gather (BASELINE config 5: 111 M nodes, degrees uniform in [0, 2 x 29],
int32 neighbour ids drawn from a power law with exponent 0.8, CHUNKED) plus one float weight per edge, 10^U(-3, 3) from a seeded
generator. Batch: 1024 seeds, fan-outs 30,30, fixed per-hop sampler seeds. One step = the call + a device synchronise. Timed
in one process, median / min / max of --steps steps after --warmup warm-up steps:
  (a) edge_chain   multilayer_sample_with_edge_attributes(["w"], weight_name="w") as the package routes it: the one-call
                   chain with edge ids, the weight fetched by edge_attr_gather_kernel behind each hop
  (b) two_op       the body that call had before the chain carried edge ids, kept here as the baseline: per hop the one-hop
                   sampler with edge output, append_unique and a WholeMemory gather of the attribute
  (c) chain        multilayer_sample_without_replacement(weight_name="w"): the chain without edge ids
Gates (booleans in the line): (a) faster than (b); (a) within (c) x (1 + added algorithmic bytes / (c)'s bytes) x ((c)'s max /
median), the run-to-run spread of the baseline being the only noise figure there is. Algorithmic bytes of a hop with n centres,
D edges under them, S samples, U unique ids out and ids of b bytes:
  (c)    n (2 b + 40)  centres, row bounds and offsets, read by the scan and by the sampler
       + 4 D           the weights of the centres' rows
       + S (2 b + 4)   columns read, ids and centre ids written
       + (n + S) (b + 20)   keys read; slot, smallest position and slot index of the hash table
       + 12 S + b U    ranks written and read, positions and unique ids written
  added  24 S          edge ids written (8) and read (8), the attribute read (4) and written (4)

--launches STEPS runs only STEPS steps of --variant and prints their number: run it under `rocprofv3 --kernel-trace --stats`
and hand the kernel stats files to a timing run with --stats-a / --stats-c, which adds the library kernels launched per step."""
import argparse
import csv
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


def two_op_body(g, node_ids, max_neighbors, edge_attr_names, weight_name, random_seeds):
    """multilayer_sample_with_edge_attributes as it was before the chain carried edge ids"""
    import torch
    from wholegraph_amd.torch import graph_ops
    hops = len(max_neighbors)
    targets, edges, rows, cols, attrs = [None] * hops + [node_ids], [None] * hops, [None] * hops, [None] * hops, [None] * hops
    frontier = node_ids
    for depth, fanout in enumerate(max_neighbors):
        offsets, neighbours, centre_lid, edge_id = g._one_hop(frontier, fanout, weight_name, random_seeds[depth], True, True)
        widened, neighbour_pos = graph_ops.append_unique(frontier, neighbours, need_neighbor_raw_to_unique=True)
        layer = hops - 1 - depth
        targets[layer], edges[layer], rows[layer], cols[layer] = widened, torch.stack([neighbour_pos, centre_lid]), offsets, neighbour_pos
        attrs[layer] = {name: edge_id if name == "__edge_id__" else g.edge_attributes[name].gather(edge_id) for name in edge_attr_names}
        frontier = widened
    return targets, edges, rows, cols, attrs


def library_launches(stats_csv, steps):
    """kernels of the library (namespace wm) per step, from a rocprofv3 kernel stats file"""
    calls = 0
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            if "wm::" in row.get("Name", ""):
                calls += int(row["Calls"])
    return round(calls / steps, 2)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=111_059_956)
    p.add_argument("--avg-degree", type=int, default=29)
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanouts", default="30,30")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--launches", type=int, default=0)
    p.add_argument("--variant", choices=["a", "c"], default="a")
    p.add_argument("--stats-a", default=None)
    p.add_argument("--stats-c", default=None)
    p.add_argument("--stats-steps", type=int, default=20)
    p.add_argument("--stats-nodes", type=int, default=2_000_000)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_chain_bench.json"))
    a = p.parse_args()
    sys.path.insert(0, ROOT)
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
    lrow = wrow.get_local_tensor()[0]
    lrow.copy_(row)
    del row
    lcol, lwgt = wcol.get_local_tensor()[0], wwgt.get_local_tensor()[0]
    genw, gen2 = torch.Generator(device="cuda").manual_seed(4242), torch.Generator(device="cuda").manual_seed(100)
    for s0 in range(0, edges, 1 << 28):
        e0 = min(edges, s0 + (1 << 28))
        lwgt[s0:e0] = torch.pow(10.0, torch.rand(e0 - s0, device="cuda", generator=genw) * 6.0 - 3.0)
        lcol[s0:e0] = powerlaw_ids(nodes, e0 - s0, 0.8, gen2)
    seeds = torch.randint(0, nodes, (a.seeds,), device="cuda", generator=gen2, dtype=torch.int32)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    g.set_edge_attribute("w", wwgt)
    torch.cuda.synchronize()

    run_a = lambda: g.multilayer_sample_with_edge_attributes(seeds, fanouts, ["w"], "w", random_seeds=hop_seeds)
    run_b = lambda: two_op_body(g, seeds, fanouts, ["w"], "w", hop_seeds)
    run_c = lambda: g.multilayer_sample_without_replacement(seeds, fanouts, "w", random_seeds=hop_seeds)
    if a.launches > 0:
        fn = run_a if a.variant == "a" else run_c
        for _ in range(a.launches):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"bench": "edge_chain_launches", "variant": a.variant, "steps": a.launches}))
        return

    calls = binding.lib().wholememory_ext_edge_chain_calls
    before = calls()
    got_a = run_a()
    route_a = "one-call chain with edge ids" if calls() == before + 1 else "hop by hop"
    got_b, got_c = run_b(), run_c()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for la, lb in zip(got_a[:4], got_b[:4]) for x, y in zip(la, lb)) and all(
        torch.equal(x["w"].view(torch.int32), y["w"].view(torch.int32)) for x, y in zip(got_a[4], got_b[4]))
    same_c = all(torch.equal(x, y) for la, lc in zip(got_a[:4], got_c) for x, y in zip(la, lc))
    tg, ci = got_a[0], got_a[3]
    b = 4
    c_bytes = added = 0
    for layer in range(len(fanouts)):
        centres = tg[layer + 1].long()
        n, S, U = int(centres.numel()), int(ci[layer].numel()), int(tg[layer].numel())
        D = int((lrow[centres + 1] - lrow[centres]).sum().item())
        c_bytes += n * (2 * b + 40) + 4 * D + S * (2 * b + 4) + (n + S) * (b + 20) + 12 * S + b * U
        added += 24 * S
    res = {"bench": "edge_chain", "nodes": nodes, "edges": edges, "seeds": a.seeds, "fanouts": fanouts, "steps": a.steps,
           "warmup": a.warmup, "neighbour_ids": "power law, exponent 0.8", "route_a": route_a,
           "frontier_sizes": [int(t.numel()) for t in tg], "sampled_edges": sum(int(c.numel()) for c in ci),
           "a_equals_b": bool(same), "a_four_lists_equal_c": bool(same_c),
           "timing": "host clock around the call + device synchronise, ms per step"}
    del got_a, got_b, got_c, tg, ci
    res["a_edge_chain"] = timed_steps(run_a, a.warmup, a.steps)
    res["b_two_op"] = timed_steps(run_b, a.warmup, a.steps)
    res["c_chain"] = timed_steps(run_c, a.warmup, a.steps)
    ma, mb, mc = (res[k]["median_ms"] for k in ("a_edge_chain", "b_two_op", "c_chain"))
    spread = res["c_chain"]["max_ms"] / mc
    allow = (1.0 + added / c_bytes) * spread
    res.update({"b_over_a": round(mb / ma, 2), "a_over_c": round(ma / mc, 3), "c_algorithmic_bytes": c_bytes,
                "added_algorithmic_bytes": added, "c_max_over_median": round(spread, 3), "a_over_c_allowed": round(allow, 3),
                "gate_a_faster_than_b": bool(ma < mb), "gate_a_within_byte_ratio_of_c": bool(ma / mc <= allow)})
    if a.stats_a and a.stats_c:
        res["library_kernel_launches_per_step"] = {"a_edge_chain": library_launches(a.stats_a, a.stats_steps),
                                                   "c_chain": library_launches(a.stats_c, a.stats_steps),
                                                   "from": "rocprofv3 --kernel-trace --stats, %d steps each, a graph of %d nodes" % (a.stats_steps, a.stats_nodes)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    for t in (wrow, wcol, wwgt):
        wgth.destroy_wholememory_tensor(t)


if __name__ == "__main__":
    main()
