#!/usr/bin/env python3
"""Timing of PinSAGE importance neighbourhoods (wholegraph_amd/torch/wholegraph_ops.py: rwr_top_neighbors ->
csrc/kernels/rwr.hip) on one MI355X; writes ONE JSON line into profiles/pinsage_bench.json (and prints it).

Graph: the graph of scripts/bench_walk.py (papers100M-shaped: `--nodes` nodes, degrees uniform in [0, 58], power-law column
ids, CHUNKED, int32 ids). Workload: n random seeds, R walks of L steps each, the T = 10 most visited nodes, for every
(n, R, L) of CONFIGS. In one process, alternating:
  fused       rwr_top_neighbors(..., restart_prob = 0.5): one launch, [n, T] ids and counts written
  floor       the same call with restart_prob = 1 - 2^-32: (nearly) every step restarts, so no graph read, no visit and no
              merge is left: the launch, the generators, the table's clear and its scan
  walks       random_walk from the n * R repeated starts, L steps: the first stage of the composition, [n * R, L + 1] ids written
  composition what a user has without the op: those walks, a torch sort of the (seed, node) keys with a segmented count
              (unique_consecutive), and a per-seed top-T by a second sort. No restarts and no dangling rule: compared for TIME only
The selection's share: at fixed n = 10 000 and R = 128 the op and the floor are also timed at L = 9 and 12, which use the same
4096-slot table as L = 16 in the same two passes. Reads, draws and counting grow with L; the clear, the scan and the top_merge
rounds do not (every 64-slot batch holds a visited node at any of these L). So the intercept of time over L is the fixed
cost of a call, the floor's intercept is the part of it without merges, and `selection` in the JSON is their difference.
`--rounds` rounds, in each the median of `--reps` calls after `--warmup`, timed with events; the result is the median over the
rounds with the lowest and highest round next to it; the ratios are formed round by round. step_ns = time / (n * R * L).

The measurement runs in a child process under `timeout` (--step-timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FIXED_N, FIXED_R, FIXED_LS = 10_000, 128, (9, 12, 16)      # one table tier, the same passes: time is linear in L
CONFIGS = ((1024, 16, 4), (10_000, 16, 4), (100_000, 16, 4), (1024, 128, 16), (10_000, 128, 16), (100_000, 128, 16))
TOP = 10


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_pinsage.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    from bench_sage_agg import timed
    from bench_walk import build_graph
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    wrow, wcol, wwgt, edges = build_graph(wgth, comm, a.nodes, 29)
    wgth.destroy_wholememory_tensor(wwgt)
    row, col = wrow.wmb_tensor, wcol.wmb_tensor
    nodes = a.nodes
    gen = torch.Generator(device="cuda").manual_seed(7)
    all_seeds = torch.randint(0, nodes, (max(c[0] for c in CONFIGS),), device="cuda", generator=gen, dtype=torch.int32)

    def composition(seeds, R, L):
        n, V = seeds.shape[0], R * L
        starts = seeds.repeat_interleave(R)
        owner = torch.arange(n, device="cuda")[:, None]

        def walks():
            return wops.random_walk(row, col, starts, L, 3)

        def fn():
            visited = walks()[:, 1:].reshape(n, V).long()
            visited = torch.where(visited == seeds.long()[:, None], -1, visited)           # (arrivals at the seed are not counted)
            keys = torch.sort((owner * (nodes + 1) + visited + 1).reshape(-1)).values
            uniq, count = torch.unique_consecutive(keys, return_counts=True)
            seg, node = uniq // (nodes + 1), uniq % (nodes + 1) - 1
            order = torch.sort(seg * (V + 1) + (V - count), stable=True).indices           # per seed: count descending, id ascending
            seg, node, count = seg[order], node[order], count[order]
            rank = torch.arange(seg.shape[0], device="cuda") - torch.searchsorted(seg, torch.arange(n, device="cuda"))[seg]
            keep = (rank < TOP) & (node >= 0)
            out_nodes = torch.full((n, TOP), -1, device="cuda", dtype=torch.int64)
            out_counts = torch.zeros((n, TOP), device="cuda", dtype=torch.int64)
            out_nodes[seg[keep], rank[keep]] = node[keep]
            out_counts[seg[keep], rank[keep]] = count[keep]
            return out_nodes, out_counts
        return walks, fn
    steps, work, filled = {}, {}, {}
    for n, R, L in CONFIGS:
        tag = "n%d_r%d_l%d" % (n, R, L)
        seeds = all_seeds[:n]
        work[tag] = n * R * L
        steps["fused_" + tag] = lambda s=seeds, R=R, L=L: wops.rwr_top_neighbors(row, col, s, R, L, 0.5, TOP, 3)
        steps["floor_" + tag] = lambda s=seeds, R=R, L=L: wops.rwr_top_neighbors(row, col, s, R, L, 1.0 - 2.0 ** -32, TOP, 3)
        if not a.no_composition:
            steps["walks_" + tag], steps["composition_" + tag] = composition(seeds, R, L)
        got_nodes, got_counts = steps["fused_" + tag]()      # every form once before anything is timed
        assert int(got_nodes.min()) >= -1 and int(got_nodes.max()) < nodes and int(got_counts.max()) <= R * L
        assert bool((got_counts[:, :-1] >= got_counts[:, 1:]).all()), "counts are not descending"
        filled[tag] = round(float((got_nodes >= 0).float().mean()), 4)
    for L in FIXED_LS[:-1]:      # (the last one is among CONFIGS)
        tag = "n%d_r%d_l%d" % (FIXED_N, FIXED_R, L)
        work[tag] = FIXED_N * FIXED_R * L
        steps["fused_" + tag] = lambda L=L: wops.rwr_top_neighbors(row, col, all_seeds[:FIXED_N], FIXED_R, L, 0.5, TOP, 3)
        steps["floor_" + tag] = lambda L=L: wops.rwr_top_neighbors(row, col, all_seeds[:FIXED_N], FIXED_R, L, 1.0 - 2.0 ** -32, TOP, 3)
    rounds = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            rounds[k].append(timed(fn, a.warmup, a.reps))
    res, ratios = {}, {}
    for k, ms in rounds.items():
        tag = k.split("_", 1)[1]
        res[k + "_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                          "step_ns": round(statistics.median(ms) * 1e6 / work[tag], 3)}
        if k.startswith("fused_"):
            for other in ("floor", "walks", "composition"):
                if other + "_" + tag in rounds:
                    r = [p / q for p, q in zip(rounds[other + "_" + tag], ms)]
                    ratios["%s_over_fused_%s" % (other, tag)] = {"median": round(statistics.median(r), 3), "min": round(min(r), 3),
                                                                "max": round(max(r), 3)}
    def intercept(kind, r):      # of the least-squares line through (L, time of round r)
        ys = [rounds["%s_n%d_r%d_l%d" % (kind, FIXED_N, FIXED_R, L)][r] for L in FIXED_LS]
        mx, my = statistics.mean(FIXED_LS), statistics.mean(ys)
        slope = sum((x - mx) * (y - my) for x, y in zip(FIXED_LS, ys)) / sum((x - mx) ** 2 for x in FIXED_LS)
        return my - slope * mx
    whole = rounds["fused_n%d_r%d_l%d" % (FIXED_N, FIXED_R, FIXED_LS[-1])]
    fixed = [(intercept("fused", r), intercept("floor", r)) for r in range(a.rounds)]
    selection = {"n": FIXED_N, "R": FIXED_R, "L": list(FIXED_LS),
                 "fused_intercept_ms": round(statistics.median(f for f, _ in fixed), 4),
                 "floor_intercept_ms": round(statistics.median(g for _, g in fixed), 4),
                 "selection_ms": round(statistics.median(f - g for f, g in fixed), 4),
                 "share_of_l%d" % FIXED_LS[-1]: round(statistics.median((f - g) / w for (f, g), w in zip(fixed, whole)), 4)}
    line = {"bench": "pinsage_neighbors", "library": os.path.relpath(binding.LIB_PATH, ROOT), "nodes": nodes, "edges": edges,
            "mean_degree": round(edges / nodes, 2), "top": TOP, "restart_prob": 0.5, "warmup": a.warmup, "reps": a.reps,
            "rounds": a.rounds, "filled": filled, "selection": selection, **res, "ratios": ratios}
    print("PINSAGE_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--no-composition", action="store_true", help="time the fused forms alone")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pinsage_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--rounds", str(a.rounds), "--nodes", str(a.nodes)]
    if a.no_composition:
        cmd.append("--no-composition")
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("PINSAGE_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_pinsage: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return child.returncode or 1
    line = lines[-1][len("PINSAGE_BENCH "):]
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
