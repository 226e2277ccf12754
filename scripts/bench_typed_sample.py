#!/usr/bin/env python3
"""Timing of per-relation fan-out neighbour sampling (wholegraph_amd/torch/wholegraph_ops.py: typed_sample_without_replacement
-> csrc/kernels/tysample.hip) on one MI355X; writes ONE JSON line into profiles/typed_sample_bench.json (and prints it).

Graph: the graph of scripts/bench_walk.py (papers100M-shaped: `--nodes` nodes, degrees uniform in [0, 58], power-law column
ids, CHUNKED, int32 ids) with an int32 relation per edge, drawn SKEWED: relation 0 holds nine edges in ten, the others share the
rest evenly; R = 4 and R = 16, one type tensor each. Centres: the node sets of scripts/bench_temporal_sample.py. Fan-outs: 8 per
relation at R = 4 (F = 32, the 32-lane select) and 4 per relation at R = 16 (F = 64, the 64-lane select). In one process,
alternating, for every set and R:
  op          typed_sample_without_replacement(..., need_edge_output=True, need_type_output=True)
  composite   what it replaces: unweighted_sample_without_replacement(..., max_sample_count=-1) with centre ids and edge ids
              (all D = sum of deg(centres) neighbours materialised, one host round trip), the types of those edges, a random key
              per edge, one sort by (centre, relation, key), the rank within the (centre, relation) segment, rank < f_r
  floor       unweighted_sample_without_replacement at fan-out F with edge ids: the plain sampler, which reads no types
The median of `--reps` calls after `--warmup`, timed with events. Before anything is timed, op and composite must agree on the
offsets and on the number of samples per relation. `rare_share`: the share of the op's samples that are not of relation 0,
beside the same share for the floor's samples: what the fan-out per relation is for.

The measurement runs in a child process under `timeout` (--step-timeout seconds); the parent never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SETS = ((3_000, 2), (20_000, 4), (100_000, 4))      # (roots, steps)
CONFIGS = ((4, 8), (16, 4))                         # (R, fan-out per relation)


def composite(wops, torch, row, col, ltype, centres, fan):
    """-> offsets int32 [n + 1], ids, edge ids, types by the four-step route; fan: int64 [R] on the device"""
    n, R = centres.shape[0], fan.shape[0]
    _, ids, lid, eid = wops.unweighted_sample_without_replacement(row, col, centres, -1, 1, True, True)
    ty = ltype[eid].long()
    live = (ty >= 0) & (ty < R)
    live &= fan[ty.clamp(0, R - 1)] > 0
    ids, eid, ty, seg = ids[live], eid[live], ty[live], lid.long()[live] * R + ty[live]
    key = torch.rand(seg.shape[0], device=seg.device, dtype=torch.float64)
    order = torch.argsort(seg.double() - key * 0.999)           # by (centre, relation), the largest key first
    counts = torch.bincount(seg, minlength=n * R)
    starts = torch.cumsum(counts, 0) - counts
    rank = torch.arange(seg.shape[0], device=seg.device) - starts[seg[order]]
    chosen = torch.sort(order[rank < fan[ty[order]]])[0]        # back into row order
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=seg.device)
    torch.cumsum(torch.minimum(counts.view(n, R), fan).sum(1), 0, out=offsets[1:])
    return offsets, ids[chosen], eid[chosen], ty[chosen]


def measure(a):
    import torch
    assert torch.cuda.is_available(), "bench_typed_sample.py measures the GPU: no GPU found"
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
    row, col, lrow = wrow.wmb_tensor, wcol.wmb_tensor, wrow.get_local_tensor()[0]
    types = {}
    for R, _ in CONFIGS:      # relation 0 with probability 0.9, else one of 1 .. R - 1
        wtype = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [edges], torch.int32, [1])
        ltype = wtype.get_local_tensor()[0]
        gen = torch.Generator(device="cuda").manual_seed(11 + R)
        for s0 in range(0, edges, 1 << 28):
            e0 = min(edges, s0 + (1 << 28))
            u = torch.rand(e0 - s0, device="cuda", generator=gen)
            ltype[s0:e0] = torch.where(u < 0.9, 0, 1 + ((u - 0.9) * 10 * (R - 1)).long().clamp(max=R - 2)).int()
            del u
        types[R] = (wtype, ltype)
    gen = torch.Generator(device="cuda").manual_seed(7)
    sets = {}
    for roots, steps in SETS:
        starts = torch.randint(0, a.nodes, (roots,), device="cuda", generator=gen, dtype=torch.int32)
        walks = wops.random_walk(row, col, starts, steps, 3)
        centres = torch.unique(walks[walks >= 0])
        deg = lrow[centres.long() + 1] - lrow[centres.long()]
        res = {"centres": int(centres.shape[0]), "D": int(deg.sum())}
        for R, f in CONFIGS:
            wtype, ltype = types[R]
            fanouts, fan = [f] * R, torch.full((R,), f, dtype=torch.int64, device="cuda")
            op = lambda: wops.typed_sample_without_replacement(row, col, wtype.wmb_tensor, centres, fanouts, 5, False, True, True)
            floor = lambda: wops.unweighted_sample_without_replacement(row, col, centres, f * R, 5, False, True)
            offsets, ids, eid, ty = op()
            torch.cuda.synchronize()
            assert int(offsets[-1]) == ids.shape[0] == eid.shape[0] and torch.equal(ltype[eid], ty)
            one = {"F": f * R, "entries": int(offsets[-1]), "rare_share": round(float((ty != 0).double().mean()), 4),
                   "floor_rare_share": round(float((ltype[floor()[2]] != 0).double().mean()), 4)}
            c_off, _, _, c_ty = composite(wops, torch, row, col, ltype, centres, fan)
            assert torch.equal(c_off, offsets), "the op and the composite disagree on the offsets"
            assert torch.equal(torch.bincount(c_ty, minlength=R), torch.bincount(ty.long(), minlength=R)), "... on the relations"
            del offsets, ids, eid, ty, c_off, c_ty
            one["op_ms"] = round(timed(op, a.warmup, a.reps), 4)
            one["composite_ms"] = round(timed(lambda: composite(wops, torch, row, col, ltype, centres, fan), a.warmup, a.reps), 4)
            one["floor_ms"] = round(timed(floor, a.warmup, a.reps), 4)
            one["composite_over_op"] = round(one["composite_ms"] / one["op_ms"], 2)
            one["op_over_floor"] = round(one["op_ms"] / one["floor_ms"], 2)
            res["R%d" % R] = one
        sets["%dx%d" % (roots, steps)] = res
    line = {"bench": "typed_sample", "library": os.path.relpath(binding.LIB_PATH, ROOT), "graph_nodes": a.nodes, "edges": edges,
            "mean_degree": round(edges / a.nodes, 2), "skew": 0.9, "warmup": a.warmup, "reps": a.reps, "sets": sets}
    print("TYSAMPLE_BENCH " + json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--nodes", type=int, default=111_059_956, help="graph nodes (bench.py sample_gather default)")
    p.add_argument("--step-timeout", type=int, default=540, help="seconds the measuring child process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "typed_sample_bench.json"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--warmup",
           str(a.warmup), "--reps", str(a.reps), "--nodes", str(a.nodes)]
    child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    lines = [l for l in child.stdout.splitlines() if l.startswith("TYSAMPLE_BENCH ")]
    if child.returncode != 0 or not lines:
        print("bench_typed_sample: the measuring step ended with status %d" % child.returncode, file=sys.stderr)
        sys.stderr.write(child.stdout[-2000:])
        return 1
    text = lines[-1][len("TYSAMPLE_BENCH "):]
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
