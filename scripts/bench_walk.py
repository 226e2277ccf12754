#!/usr/bin/env python3
"""Timing of fused random walks (wholegraph_amd/torch/wholegraph_ops.py: random_walk -> csrc/kernels/walk.hip) on one MI355X;
writes ONE JSON line into profiles/walk_bench.json (and prints it).

Graph: the synthetic papers100M-shaped graph of bench.py's sample_gather workload (scripts/bench_sage_agg.py builds the same:
`--nodes` nodes, degrees uniform in [0, 58], power-law column ids, CHUNKED, int32 ids), plus one fp32 weight per edge,
uniform in (0, 1]. Workload: `--walks` walks of `--length` steps from random start nodes. In one process, alternating:
  uniform      random_walk(...)                                   one launch, no host round trip
  weighted     random_walk(..., wm_csr_weight_ptr_tensor=w)       one launch, no host round trip
  hop_by_hop   the only composition available without the fused op: `--length` calls of
               unweighted_sample_without_replacement(..., max_sample_count=1) on the walks still alive, each ragged output
               re-padded into the [n, L + 1] array (one library call, one scan and one host round trip per step)
`--rounds` rounds, in each the median of `--reps` calls of the fused forms and of `--slow-reps` calls of the composition after
`--warmup`; the result is the median over the rounds with the lowest and highest round next to it, the ratios are formed
round by round. steps_per_s counts the n * L steps asked for; `taken` is the share of them that a walk took (a walk that
reaches a node without neighbours ends). ns_per_step is the time of the uniform call over L: what one step of every walk
costs, to be set against two dependent memory round trips (row_ptr, then col_ind; ~900 cycles each on a miss to HBM).

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


def build_graph(wgth, comm, nodes, avg):
    """-> (row, col, weight) CHUNKED WholeMemory tensors; the structure of bench_sage_agg.c5_layer0's graph"""
    import torch
    from bench_sage_agg import powerlaw_ids
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
    gen2 = torch.Generator(device="cuda").manual_seed(100)
    for s0 in range(0, edges, 1 << 28):
        e0 = min(edges, s0 + (1 << 28))
        lcol[s0:e0] = powerlaw_ids(nodes, e0 - s0, 0.8, gen2)
        lwgt[s0:e0] = 1.0 - torch.rand(e0 - s0, device="cuda", generator=gen2)
    torch.cuda.synchronize()
    return wrow, wcol, wwgt, edges


def hop_by_hop(wops, row, col, starts, length, seed):
    """the walk as `length` one-neighbour hops, the ragged result of each re-padded: [n, length + 1], -1 behind a walk's end"""
    import torch
    n = starts.shape[0]
    walks = torch.full((n, length + 1), -1, dtype=starts.dtype, device=starts.device)
    walks[:, 0] = starts
    alive, cur = torch.arange(n, device=starts.device), starts
    for t in range(length):
        if cur.numel() == 0:
            break
        off, ids = wops.unweighted_sample_without_replacement(row, col, cur, 1, seed + t)
        moved = (off[1:] - off[:-1]) > 0
        alive = alive[moved]
        walks[alive, t + 1] = ids
        cur = ids
    return walks


def check_walks(walks, eids, row, col, n_nodes):
    """every step taken is an edge of the node it leaves; -1 from a walk's end on, in both outputs"""
    import torch
    taken = eids >= 0
    assert torch.equal(taken, walks[:, 1:] >= 0)
    assert not bool((taken[:, 1:] & ~taken[:, :-1]).any())
    src = walks[:, :-1][taken].long()
    e = eids[taken]
    assert bool(((e >= row[src]) & (e < row[src + 1])).all()) and torch.equal(col[e], walks[:, 1:][taken])
    return float(taken.float().mean())


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_walk.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from bench_sage_agg import timed
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    wrow, wcol, wwgt, edges = build_graph(wgth, comm, a.nodes, 29)
    row, col, wgt = wrow.wmb_tensor, wcol.wmb_tensor, wwgt.wmb_tensor
    gen = torch.Generator(device="cuda").manual_seed(7)
    starts = torch.randint(0, a.nodes, (a.walks,), device="cuda", generator=gen, dtype=torch.int32)
    n, L = a.walks, a.length
    # the fused forms on this graph, before anything is timed
    lrow, lcol = wrow.get_local_tensor()[0], wcol.get_local_tensor()[0]
    taken = {}
    for name, w in (("uniform", None), ("weighted", wgt)):
        walks, eids = wops.random_walk(row, col, starts, L, 3, wm_csr_weight_ptr_tensor=w, need_edge_output=True)
        taken[name] = round(check_walks(walks, eids, lrow, lcol, a.nodes), 4)
    ref = hop_by_hop(wops, row, col, starts, L, 3)
    taken["hop_by_hop"] = round(float((ref[:, 1:] >= 0).float().mean()), 4)
    del walks, eids, ref
    steps = {
        "uniform": (lambda: wops.random_walk(row, col, starts, L, 3), a.warmup, a.reps),
        "weighted": (lambda: wops.random_walk(row, col, starts, L, 3, wm_csr_weight_ptr_tensor=wgt), a.warmup, a.reps),
        "hop_by_hop": (lambda: hop_by_hop(wops, row, col, starts, L, 3), 1, a.slow_reps),
    }
    rounds = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, (fn, warmup, reps) in steps.items():
            rounds[k].append(timed(fn, warmup, reps))
    res = {}
    for k, ms in rounds.items():
        res[k + "_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        res[k + "_steps_per_s"] = round(n * L / statistics.median(ms) * 1e3)

    def ratio(num, den):
        r = [p / q for p, q in zip(rounds[num], rounds[den])]
        return {"median": round(statistics.median(r), 2), "min": round(min(r), 2), "max": round(max(r), 2)}
    res["ratios"] = {"hop_by_hop_over_uniform": ratio("hop_by_hop", "uniform"),
                     "weighted_over_uniform": ratio("weighted", "uniform")}
    ns_per_step = statistics.median(rounds["uniform"]) * 1e6 / L
    line = {"bench": "walk", "nodes": a.nodes, "edges": edges, "mean_degree": round(edges / a.nodes, 2), "walks": n, "length": L,
            "warmup": a.warmup, "reps": a.reps, "slow_reps": a.slow_reps, "rounds": a.rounds, "taken": taken,
            "uniform_ns_per_step": round(ns_per_step, 1), "two_hbm_misses_ns": round(2 * 900 / 2.4, 1), **res}
    print("WALK_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--slow-reps", type=int, default=3, help="calls of the hop-by-hop composition per round")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--walks", type=int, default=100_000)
    p.add_argument("--length", type=int, default=80)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--slow-reps", str(a.slow_reps), "--rounds", str(a.rounds), "--walks",
           str(a.walks), "--length", str(a.length), "--nodes", str(a.nodes)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("WALK_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_walk: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return child.returncode or 1
    line = lines[-1][len("WALK_BENCH "):]
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
