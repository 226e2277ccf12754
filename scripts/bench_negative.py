#!/usr/bin/env python3
"""Timing of fused negative sampling (wholegraph_amd/torch/wholegraph_ops.py: negative_sample -> csrc/kernels/neg_sample.hip) on
one MI355X; writes ONE JSON line into profiles/neg_bench.json (and prints it).

Graph: the graph of scripts/bench_walk.py (papers100M-shaped: `--nodes` nodes, degrees uniform in [0, 58], power-law column
ids, CHUNKED, int32 ids) with every row of col_ind sorted ascending once, before anything is timed. Workload: `--sources`
random source nodes, K = 5 and K = 20 negatives each, neighbours and the source excluded, the default 8 tries. In one process,
alternating, for both K and both modes:
  fused_scan     negative_sample(..., col_sorted=False): one launch, the group scans the source's row
  fused_search   negative_sample(..., col_sorted=True): one launch, a binary search per candidate
  torch          the composition available without the op, on plain torch tensors: torch.randint candidates (mode "degree":
                 col_ind at torch.randint positions), membership by torch.searchsorted over the sorted key array
                 u * n_nodes + c of all edges (built before anything is timed: with ascending rows the edges in CSR order ARE
                 that sorted array), ONE redraw round for the rejected candidates, -1 where the redrawn candidate is rejected
                 too. It never leaves the device and never synchronises, so its second membership test runs over all n * K.
                 (It needs the 8-byte key per edge next to the graph, and a graph that torch can index: a flat device tensor.)
`--rounds` rounds, in each the median of `--reps` calls after `--warmup`, timed with events; the result is the median over the
rounds with the lowest and highest round next to it; the ratio torch / fused is formed round by round. `minus` is the share of
outputs that are -1. `--no-composition` times the fused forms alone (the runs that compare builds of the kernel).

The measurement runs in a child process under `timeout` (--step-timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)   # (behind PYTHONPATH: a variant build of scripts/build_variant.sh is measured with PYTHONPATH=experiments/variants/NAME)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

KS = (5, 20)
MODES = ("uniform", "degree")


def edge_keys(row, col, nodes, chunk_rows=1 << 22):
    """-> int64 [edges]: u * nodes + col_ind[e] for every edge e of source u, in CSR order (ascending when the rows are)"""
    import torch
    keys = torch.empty(col.shape[0], dtype=torch.int64, device=col.device)
    for r0 in range(0, nodes, chunk_rows):
        r1 = min(nodes, r0 + chunk_rows)
        s0, e0 = int(row[r0]), int(row[r1])
        owner = torch.repeat_interleave(torch.arange(r0, r1, device=col.device), row[r0 + 1:r1 + 1] - row[r0:r1])
        keys[s0:e0] = owner * nodes + col[s0:e0].long()
        del owner
    return keys


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_negative.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding            # (first: the helper scripts below put the repository in front of PYTHONPATH)
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    from bench_node2vec import sort_rows
    from bench_sage_agg import timed
    from bench_walk import build_graph
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    wrow, wcol, wwgt, edges = build_graph(wgth, comm, a.nodes, 29)
    wgth.destroy_wholememory_tensor(wwgt)
    row, col = wrow.wmb_tensor, wcol.wmb_tensor
    lrow, lcol = wrow.get_local_tensor()[0], wcol.get_local_tensor()[0]
    sort_rows(lrow, lcol)
    torch.cuda.synchronize()
    nodes, n = a.nodes, a.sources
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(0, nodes, (n,), device="cuda", generator=gen, dtype=torch.int32)
    src64 = src.long()[:, None]
    keys = edge_keys(lrow, lcol, nodes)
    torch.cuda.synchronize()
    probe = torch.randint(0, edges - 1, (1 << 20,), device="cuda")
    assert bool((keys[probe] <= keys[probe + 1]).all()), "the key array is not ascending"

    def rejected(c):
        """[n, K] bool: c is the source or one of its neighbours"""
        key = (src64 * nodes + c).reshape(-1)
        pos = torch.searchsorted(keys, key).clamp_(max=edges - 1)
        return (keys[pos] == key).reshape(c.shape) | (c == src64)

    def fused(k, mode, col_sorted):
        return lambda: wops.negative_sample(row, col, src, k, 3, mode=mode, col_sorted=col_sorted)

    def composition(k, mode):
        def draw():
            if mode == "uniform":
                return torch.randint(0, nodes, (n, k), device="cuda")
            return lcol[torch.randint(0, edges, (n, k), device="cuda")].long()

        def fn():
            c = draw()
            c = torch.where(rejected(c), draw(), c)
            return torch.where(rejected(c), -1, c)
        return fn
    steps, minus = {}, {}
    for k in KS:
        for mode in MODES:
            tag = "%s_k%d" % (mode, k)
            steps["fused_scan_" + tag] = fused(k, mode, False)
            steps["fused_search_" + tag] = fused(k, mode, True)
            if not a.no_composition:
                steps["torch_" + tag] = composition(k, mode)
            # every form on this graph before anything is timed: the routes agree, nothing drawn is excluded
            scan, search = steps["fused_scan_" + tag]().long(), steps["fused_search_" + tag]().long()
            assert torch.equal(scan, search), "the two search routes disagree: " + tag
            assert int(scan.min()) >= -1 and int(scan.max()) < nodes
            assert not bool((rejected(scan) & (scan >= 0)).any()), "a negative is the source or a neighbour: " + tag
            minus["fused_" + tag] = round(float((scan < 0).float().mean()), 6)
            if not a.no_composition:
                out = steps["torch_" + tag]()
                assert not bool((rejected(out) & (out >= 0)).any())
                minus["torch_" + tag] = round(float((out < 0).float().mean()), 6)
            del scan, search
    rounds = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            rounds[k].append(timed(fn, a.warmup, a.reps))
    res, ratios = {}, {}
    for k, ms in rounds.items():
        res[k + "_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        if k.startswith("fused_") and not a.no_composition:
            r = [p / q for p, q in zip(rounds["torch_" + k.split("_", 2)[2]], ms)]
            ratios["torch_over_" + k] = {"median": round(statistics.median(r), 2), "min": round(min(r), 2), "max": round(max(r), 2)}
    line = {"bench": "negative_sample", "library": os.path.relpath(binding.LIB_PATH, ROOT), "nodes": nodes, "edges": edges,
            "mean_degree": round(edges / nodes, 2), "sources": n, "max_tries": 8, "warmup": a.warmup, "reps": a.reps,
            "rounds": a.rounds, "minus": minus, **res, "ratios": ratios}
    print("NEG_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--sources", type=int, default=100_000)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--no-composition", action="store_true", help="time the fused forms alone")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "neg_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--rounds", str(a.rounds), "--sources", str(a.sources), "--nodes", str(a.nodes)]
    if a.no_composition:
        cmd.append("--no-composition")
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("NEG_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_negative: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return child.returncode or 1
    line = lines[-1][len("NEG_BENCH "):]
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
