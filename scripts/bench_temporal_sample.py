#!/usr/bin/env python3
"""Timing of temporal neighbour sampling (wholegraph_amd/torch/wholegraph_ops.py: temporal_sample_without_replacement ->
csrc/kernels/tsample.hip) on one MI355X; writes ONE JSON line into profiles/temporal_sample_bench.json (and prints it).

Graph: the graph of scripts/bench_walk.py (papers100M-shaped: `--nodes` nodes, degrees uniform in [0, 58], power-law column
ids, CHUNKED, int32 ids) with an int64 time per edge, uniform in [0, 10^6). Centres: the node sets of
scripts/bench_induced_subgraph.py (the sorted distinct nodes of uniform walks from 3 000 roots x 2 steps, 20 000 x 4 and
100 000 x 4), every centre at the median time 500 000. Fan-outs 10 and 30, both strategies. In one process, alternating, for
every set and fan-out:
  op          temporal_sample_without_replacement(..., need_edge_output=True): count, scan, one host round trip, select
  composite   what it replaces: unweighted_sample_without_replacement(..., max_sample_count=-1) with centre ids and edge ids
              (all D = sum of deg(centres) neighbours materialised, one host round trip), the times of those edges, the mask,
              and a per-segment top-k in torch: a key per kept edge (random, or the time for "last"), one sort by (centre, key),
              the rank within the segment from the counts, rank < M
  floor       unweighted_sample_without_replacement at the same fan-out with edge ids: the same op without the timestamp reads
The median of `--reps` calls after `--warmup`, timed with events. `GBps` is the op's effective bandwidth over a traffic model
of 16 B per row entry (the timestamp is read by the count and again by the select) plus 16 B per centre (id and time) and, per
output entry, the column id read and written and the int64 edge id. Before anything is timed, op and composite must agree on
the offsets and, for "last" (where the choice does not depend on the draws), on the edge ids up to ties in time.
`hub_share`: the share of D that lies in rows of more than 64 entries (none on this graph). `hub_rows`: the op on a second,
small graph that has hub rows, with and without the hub centres of one batch (see hub_rows below).

Every measurement runs in a child process under `timeout` (--step-timeout seconds); the parent never opens the GPU."""
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
FANOUTS = (10, 30)
T_MAX, T_CENTRE = 1_000_000, 500_000


def composite(wops, torch, row, col, ltime, centres, times, m, strategy):
    """-> offsets int32 [n + 1], ids, edge ids by the four-step route"""
    n = centres.shape[0]
    _, ids, lid, eid = wops.unweighted_sample_without_replacement(row, col, centres, -1, 1, True, True)
    lid = lid.long()
    ts = ltime[eid]
    keep = ts <= times[lid]
    ids, lid, eid, ts = ids[keep], lid[keep], eid[keep], ts[keep]
    key = torch.rand(lid.shape[0], device=lid.device, dtype=torch.float64) if strategy == "uniform" else ts.double() / T_MAX
    order = torch.argsort(lid.double() - key * 0.999)          # by centre, the largest key first
    lid_sorted = lid[order]
    counts = torch.bincount(lid, minlength=n)
    starts = torch.cumsum(counts, 0) - counts
    rank = torch.arange(lid.shape[0], device=lid.device) - starts[lid_sorted]
    chosen = torch.sort(order[rank < m])[0]                    # back into row order
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=lid.device)
    torch.cumsum(counts.clamp(max=m), 0, out=offsets[1:])
    return offsets, ids[chosen], eid[chosen]


def hub_rows(torch, wops, timed, a):
    """What hub rows cost, on a graph that has some (the bench graph has no row above 58 entries): 200 000 nodes with degrees
    uniform in [0, 58], every 200th node a hub of 5000 entries, as plain device tensors; 20 000 drawn centres at the median
    time, fan-out 30, uniform. The op on all of them and on the same batch without its hubs: hub_time_share = 1 - without /
    with, beside the hubs' share of the row entries. A failure here is recorded, not raised: the other numbers stand."""
    try:
        from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
        n_nodes, gen = 200_000, torch.Generator(device="cuda").manual_seed(13)
        deg = torch.randint(0, 59, (n_nodes,), device="cuda", generator=gen)
        deg[::200] = 5000
        row = torch.zeros(n_nodes + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(deg, 0, out=row[1:])
        edges = int(row[-1])
        col = torch.randint(0, n_nodes, (edges,), device="cuda", generator=gen, dtype=torch.int32)
        tim = torch.randint(0, T_MAX, (edges,), device="cuda", generator=gen)
        hold = [wrap_torch_tensor(t) for t in (row, col, tim)]
        centres = torch.randint(0, n_nodes, (20_000,), device="cuda", generator=gen, dtype=torch.int32)
        plain = centres[centres % 200 != 0]
        out = {"nodes": n_nodes, "edges": edges, "centres": int(centres.shape[0]), "hub_centres": int(centres.shape[0] - plain.shape[0])}
        d_all, d_plain = int(deg[centres.long()].sum()), int(deg[plain.long()].sum())
        out["hub_entry_share"] = round(1 - d_plain / d_all, 4)
        for strategy in ("uniform", "last"):
            ms = []
            for batch in (centres, plain):
                times = torch.full((batch.shape[0],), T_CENTRE, dtype=torch.int64, device="cuda")
                ms.append(timed(lambda: wops.temporal_sample_without_replacement(*[h.handle for h in hold], batch, times, 30, 5, False,
                                                                                   True, strategy=strategy), a.warmup, a.reps))
            out[strategy] = {"with_hubs_ms": round(ms[0], 4), "without_hubs_ms": round(ms[1], 4),
                             "hub_time_share": round(1 - ms[1] / ms[0], 4)}
        return out
    except Exception as e:      # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_temporal_sample.py measures the GPU: no GPU found"
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
    wtime = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [edges], torch.int64, [1])
    ltime = wtime.get_local_tensor()[0]
    gen = torch.Generator(device="cuda").manual_seed(11)
    for s0 in range(0, edges, 1 << 28):
        e0 = min(edges, s0 + (1 << 28))
        ltime[s0:e0] = torch.randint(0, T_MAX, (e0 - s0,), device="cuda", generator=gen)
    row, col, tim = wrow.wmb_tensor, wcol.wmb_tensor, wtime.wmb_tensor
    lrow = wrow.get_local_tensor()[0]
    gen = torch.Generator(device="cuda").manual_seed(7)
    sets = {}
    for roots, steps in SETS:
        starts = torch.randint(0, a.nodes, (roots,), device="cuda", generator=gen, dtype=torch.int32)
        walks = wops.random_walk(row, col, starts, steps, 3)
        centres = torch.unique(walks[walks >= 0])
        times = torch.full((centres.shape[0],), T_CENTRE, dtype=torch.int64, device="cuda")
        deg = lrow[centres.long() + 1] - lrow[centres.long()]
        d, n = int(deg.sum()), int(centres.shape[0])
        res = {"centres": n, "D": d, "hub_share": round(float(deg[deg > 64].sum()) / max(d, 1), 5)}
        for m in FANOUTS:
            for strategy in ("uniform", "last"):
                op = lambda: wops.temporal_sample_without_replacement(row, col, tim, centres, times, m, 5, False, True,
                                                                      strategy=strategy)
                offsets, ids, eid = op()
                torch.cuda.synchronize()
                total = int(offsets[-1])
                assert total == ids.shape[0] == eid.shape[0] and bool((ltime[eid] <= T_CENTRE).all())
                one = {"entries": total}
                if not a.no_composition:
                    c_off, c_ids, c_eid = composite(wops, torch, row, col, ltime, centres, times, m, strategy)
                    assert torch.equal(c_off, offsets), "the op and the composite disagree on the offsets"
                    if strategy == "last":      # (the same edges up to ties in time: the sums of the chosen times agree)
                        assert int(ltime[c_eid].sum()) == int(ltime[eid].sum()), "the op and the composite disagree on the latest edges"
                    del c_off, c_ids, c_eid
                del offsets, ids, eid
                one["op_ms"] = round(timed(op, a.warmup, a.reps), 4)
                traffic = 16 * d + 16 * n + total * (2 * 4 + 8)
                one["GBps"] = round(traffic / one["op_ms"] / 1e6, 1)
                if not a.no_composition:
                    one["composite_ms"] = round(timed(lambda: composite(wops, torch, row, col, ltime, centres, times, m, strategy),
                                                      a.warmup, a.reps), 4)
                    one["composite_over_op"] = round(one["composite_ms"] / one["op_ms"], 2)
                    if strategy == "uniform":
                        one["floor_ms"] = round(timed(lambda: wops.unweighted_sample_without_replacement(row, col, centres, m, 5, False, True),
                                                      a.warmup, a.reps), 4)
                        one["op_over_floor"] = round(one["op_ms"] / one["floor_ms"], 2)
                res["M%d_%s" % (m, strategy)] = one
        sets["%dx%d" % (roots, steps)] = res
    hubs = hub_rows(torch, wops, timed, a)
    line = {"bench": "temporal_sample", "hub_rows": hubs, "library": os.path.relpath(binding.LIB_PATH, ROOT), "graph_nodes": a.nodes, "edges": edges,
            "mean_degree": round(edges / a.nodes, 2), "warmup": a.warmup, "reps": a.reps, "sets": sets}
    print("TSAMPLE_BENCH " + json.dumps(line), flush=True)


def run_child(a):
    """one measuring process; -> its JSON line as a dict, or None"""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--nodes", str(a.nodes)]
    if a.no_composition:
        cmd.append("--no-composition")
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("TSAMPLE_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_temporal_sample: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return None
    return json.loads(lines[-1][len("TSAMPLE_BENCH "):])


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--no-composition", action="store_true", help="time the op alone")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_sample_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    line = run_child(a)
    if line is None:
        return 1
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
