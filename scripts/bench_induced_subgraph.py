#!/usr/bin/env python3
"""Timing of the node-induced subgraph (wholegraph_amd/torch/wholegraph_ops.py: induced_subgraph -> csrc/kernels/isub.hip) on
one MI355X; writes ONE JSON line into profiles/induced_subgraph_bench.json (and prints it).

Graph: the graph of scripts/bench_walk.py (papers100M-shaped: `--nodes` nodes, degrees uniform in [0, 58], power-law column
ids, CHUNKED, int32 ids). Node sets: the sorted distinct nodes of the op's own uniform walks (what
GraphStructure.saint_random_walk_subgraph feeds it), from 3 000 roots x 2 steps, 20 000 roots x 4 steps and 100 000 roots x 4
steps. In one process, alternating, for every set:
  op          induced_subgraph(row, col, nodes): table, count, scan, one host round trip, fill
  composite   what it replaces: unweighted_sample_without_replacement(..., max_sample_count=-1) with the centre of every
              neighbour (all D = sum of deg(nodes) neighbour ids materialised, one host round trip), torch.searchsorted of
              them over the sorted set, the mask, torch.bincount + cumsum for the offsets. The set is sorted and distinct, so
              the position the search returns IS the local id: the composite needs no second map.
The median of `--reps` calls after `--warmup`, timed with events. `kept` is m / D, the share of the neighbour ids read that
survive. Before anything is timed the two forms must agree on offsets and col.

`--groups 8,16,32,64`: for every G with a variant build experiments/variants/isub_gG (scripts/build_variant.sh isub_gG
"-DWM_ISUB_GROUP=G") the op alone is timed against that library in a process of its own, and the times are recorded under
"group_sweep": how kIsubGroup of isub.hip was chosen.

Every measurement runs in a child process under `timeout` (--step-timeout seconds), one after the other, and the first that
fails ends the run; the parent never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.environ.get("WHOLEGRAPH_AMD_VARIANT"):   # scripts/build_variant.sh NAME: a compile-time variant of the library
    sys.path.insert(0, os.path.join(ROOT, "experiments", "variants", os.environ["WHOLEGRAPH_AMD_VARIANT"]))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SETS = ((3_000, 2), (20_000, 4), (100_000, 4))      # (roots, steps)


def composite(wops, torch, row, col, nodes):
    """-> offsets int32 [n + 1], col int32 [m] by the three-step route; `nodes` sorted and distinct"""
    n = nodes.shape[0]
    _, ids, lid = wops.unweighted_sample_without_replacement(row, col, nodes, -1, 1, True, False)
    pos = torch.searchsorted(nodes, ids).clamp_(max=n - 1)
    keep = nodes[pos] == ids
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=nodes.device)
    torch.cumsum(torch.bincount(lid[keep], minlength=n), 0, out=offsets[1:])
    return offsets, pos[keep].int()


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_induced_subgraph.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding            # (first: the helper scripts below put the repository in front of the path)
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    from bench_sage_agg import timed
    from bench_walk import build_graph
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    wrow, wcol, wwgt, edges = build_graph(wgth, comm, a.nodes, 29)
    wgth.destroy_wholememory_tensor(wwgt)
    row, col = wrow.wmb_tensor, wcol.wmb_tensor
    lrow = wrow.get_local_tensor()[0]
    gen = torch.Generator(device="cuda").manual_seed(7)
    sets = {}
    for roots, steps in SETS:
        starts = torch.randint(0, a.nodes, (roots,), device="cuda", generator=gen, dtype=torch.int32)
        walks = wops.random_walk(row, col, starts, steps, 3)
        nodes = torch.unique(walks[walks >= 0])
        tag = "%dx%d" % (roots, steps)
        offsets, out_col = wops.induced_subgraph(row, col, nodes)
        torch.cuda.synchronize()
        d = int((lrow[nodes.long() + 1] - lrow[nodes.long()]).sum())
        m = int(offsets[-1])
        assert m == out_col.shape[0] and 0 <= int(out_col.min()) and int(out_col.max()) < nodes.shape[0]
        res = {"nodes": int(nodes.shape[0]), "D": d, "m": m, "kept": round(m / max(d, 1), 5)}
        if not a.no_composition:
            c_off, c_col = composite(wops, torch, row, col, nodes)
            assert torch.equal(c_off, offsets) and torch.equal(c_col, out_col), "the op and the composite disagree: " + tag
            del c_off, c_col
        del offsets, out_col
        res["op_ms"] = round(timed(lambda: wops.induced_subgraph(row, col, nodes), a.warmup, a.reps), 4)
        res["op_edge_ids_ms"] = round(timed(lambda: wops.induced_subgraph(row, col, nodes, need_edge_output=True), a.warmup, a.reps), 4)
        if not a.no_composition:
            res["composite_ms"] = round(timed(lambda: composite(wops, torch, row, col, nodes), a.warmup, a.reps), 4)
            res["composite_over_op"] = round(res["composite_ms"] / res["op_ms"], 2)
        sets[tag] = res
    line = {"bench": "induced_subgraph", "library": os.path.relpath(binding.LIB_PATH, ROOT), "graph_nodes": a.nodes, "edges": edges,
            "mean_degree": round(edges / a.nodes, 2), "warmup": a.warmup, "reps": a.reps, "sets": sets}
    print("ISUB_BENCH " + json.dumps(line), flush=True)


def run_child(a, variant, no_composition):
    """one measuring process; -> its JSON line as a dict, or None"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--nodes", str(a.nodes)]
    if no_composition:
        cmd.append("--no-composition")
    env = dict(os.environ)
    env.pop("WHOLEGRAPH_AMD_VARIANT", None)
    if variant:
        env["WHOLEGRAPH_AMD_VARIANT"] = variant
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = [l for l in child.stdout.splitlines() if l.startswith("ISUB_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_induced_subgraph: the measuring step (%s) ended with status %d" % (variant or "product", child.returncode),
              file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return None
    return json.loads(lines[-1][len("ISUB_BENCH "):])


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--no-composition", action="store_true", help="time the op alone")
    p.add_argument("--groups", default="", help="comma-separated group sizes whose variant builds are timed as well")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds a measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "induced_subgraph_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    line = run_child(a, None, a.no_composition)
    if line is None:
        return 1
    sweep = {}
    for g in [int(x) for x in a.groups.split(",") if x]:
        name = "isub_g%d" % g
        if not os.path.exists(os.path.join(ROOT, "experiments", "variants", name, "wholegraph_amd", "libwholegraph.so")):
            print("bench_induced_subgraph: no variant build %s, skipped" % name, file=sys.stderr)
            continue
        got = run_child(a, name, True)
        if got is None:       # (nothing more is started on the GPU after a step that failed)
            return 1
        sweep[str(g)] = {tag: {"op_ms": s["op_ms"], "op_edge_ids_ms": s["op_edge_ids_ms"]} for tag, s in got["sets"].items()}
    if sweep:
        line["group_sweep"] = sweep
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
