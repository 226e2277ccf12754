#!/usr/bin/env python3
"""Timing of node2vec (p, q) walks (wholegraph_amd/torch/wholegraph_ops.py: node2vec_walk -> csrc/kernels/walk_n2v.hip) on one
MI355X; writes ONE JSON line into profiles/node2vec_bench.json (and prints it).

Graph: the graph of scripts/bench_walk.py (papers100M-shaped: `--nodes` nodes, degrees uniform in [0, 58], power-law column
ids, CHUNKED, int32 ids, one fp32 weight per edge, uniform in (0, 1]) with every row of col_ind sorted ascending once, before
anything is timed (the weights are independent draws, so they are not carried along). Workload: `--walks` walks of `--length`
steps from random start nodes. In one process, alternating, each form with and without the weight tensor:
  weighted_walk        random_walk(..., weight): the first-order walk, which makes the same picks at p = q = 1 — the
                       baseline. (Without weights the baseline is still the weighted walk: the first-order walk that makes
                       the same picks as the unweighted node2vec call is the one over a tensor of ones.)
  n2v_1_1              node2vec_walk at (1, 1): no search (1 / q == 1), the class test x == u alone
  n2v_search           node2vec_walk at (0.25, 4), col_sorted=True: a binary search of the previous node's row per neighbour
  n2v_scan             node2vec_walk at (0.25, 4), col_sorted=False: the group scans the previous node's row per batch
  n2v_2_1              node2vec_walk at (2, 1): the skipped-search path with a bias that is not 1
`--rounds` rounds, in each the median of `--reps` calls after `--warmup`; the result is the median over the rounds with the
lowest and highest round next to it, the ratios to the weighted walk are formed round by round. `taken` is the share of the
n * L steps that a walk took.

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


def sort_rows(row, col, chunk_edges=1 << 27):
    """sorts every row of col (int32, non-negative) ascending, in place, a run of whole rows at a time"""
    import torch
    nodes, edges = row.shape[0] - 1, col.shape[0]
    r0 = 0
    while r0 < nodes:
        target = torch.tensor([int(row[r0]) + chunk_edges], device=row.device)
        r1 = min(nodes, max(r0 + 1, int(torch.searchsorted(row, target, right=True)) - 1))
        s0, e0 = int(row[r0]), int(row[r1])
        if e0 > s0:
            owner = torch.repeat_interleave(torch.arange(r1 - r0, device=row.device), row[r0 + 1:r1 + 1] - row[r0:r1])
            keys = (owner << 32) | col[s0:e0].long()
            del owner
            keys = torch.sort(keys).values
            col[s0:e0] = (keys & 0xFFFFFFFF).int()
            del keys
        r0 = r1
    assert edges == int(row[-1])


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_node2vec.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding            # (first: the helper scripts below put the repository in front of PYTHONPATH)
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    from bench_sage_agg import timed
    from bench_walk import build_graph, check_walks
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    wrow, wcol, wwgt, edges = build_graph(wgth, comm, a.nodes, 29)
    row, col, wgt = wrow.wmb_tensor, wcol.wmb_tensor, wwgt.wmb_tensor
    lrow, lcol = wrow.get_local_tensor()[0], wcol.get_local_tensor()[0]
    sort_rows(lrow, lcol)
    torch.cuda.synchronize()
    probe = torch.randint(0, a.nodes, (4096,), device="cuda")
    for v in probe.tolist()[:256]:
        r = lcol[int(lrow[v]):int(lrow[v + 1])]
        assert bool((r[1:] >= r[:-1]).all()), "row %d is not ascending" % v
    gen = torch.Generator(device="cuda").manual_seed(7)
    starts = torch.randint(0, a.nodes, (a.walks,), device="cuda", generator=gen, dtype=torch.int32)
    n, L = a.walks, a.length

    def n2v(p, q, col_sorted, w):
        return lambda **kw: wops.node2vec_walk(row, col, starts, L, p, q, 3, wm_csr_weight_ptr_tensor=w, col_sorted=col_sorted, **kw)
    forms = {}
    for tag, w in (("weighted", wgt), ("unweighted", None)):
        forms["n2v_1_1_" + tag] = n2v(1.0, 1.0, True, w)
        forms["n2v_search_" + tag] = n2v(0.25, 4.0, True, w)
        forms["n2v_scan_" + tag] = n2v(0.25, 4.0, False, w)
        forms["n2v_2_1_" + tag] = n2v(2.0, 1.0, True, w)
    # every form on this graph before anything is timed: the walks follow edges, both routes agree, (1, 1) is the baseline's walk
    taken = {}
    base = wops.random_walk(row, col, starts, L, 3, wm_csr_weight_ptr_tensor=wgt, need_edge_output=True)
    taken["weighted_walk"] = round(check_walks(base[0], base[1], lrow, lcol, a.nodes), 4)
    for k, fn in forms.items():
        walks, eids = fn(need_edge_output=True)
        taken[k] = round(check_walks(walks, eids, lrow, lcol, a.nodes), 4)
        if k == "n2v_1_1_weighted":
            assert torch.equal(walks, base[0]) and torch.equal(eids, base[1]), "p = q = 1 is not the weighted walk"
        if k.startswith("n2v_search_"):
            kept = walks, eids
        if k.startswith("n2v_scan_"):
            assert torch.equal(walks, kept[0]) and torch.equal(eids, kept[1]), "the two search routes disagree"
    del walks, eids, base, kept
    steps = {"weighted_walk": lambda: wops.random_walk(row, col, starts, L, 3, wm_csr_weight_ptr_tensor=wgt)}
    steps.update(forms)
    rounds = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            rounds[k].append(timed(fn, a.warmup, a.reps))
    res, ratios = {}, {}
    for k, ms in rounds.items():
        res[k + "_ms"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        if k != "weighted_walk":
            r = [p / q for p, q in zip(ms, rounds["weighted_walk"])]
            ratios[k + "_over_weighted_walk"] = {"median": round(statistics.median(r), 2), "min": round(min(r), 2),
                                                 "max": round(max(r), 2)}
    line = {"bench": "node2vec", "library": os.path.relpath(binding.LIB_PATH, ROOT), "nodes": a.nodes, "edges": edges, "mean_degree": round(edges / a.nodes, 2), "walks": n,
            "length": L, "warmup": a.warmup, "reps": a.reps, "rounds": a.rounds, "taken": taken, **res, "ratios": ratios}
    print("N2V_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--walks", type=int, default=100_000)
    p.add_argument("--length", type=int, default=80)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "node2vec_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--rounds", str(a.rounds), "--walks", str(a.walks), "--length", str(a.length),
           "--nodes", str(a.nodes)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("N2V_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_node2vec: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return child.returncode or 1
    line = lines[-1][len("N2V_BENCH "):]
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
