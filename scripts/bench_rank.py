#!/usr/bin/env python3
"""Timing of rank_rows (wholegraph_amd/torch/wholegraph_ops.py -> csrc/kernels/rank.hip) on one MI355X against the torch
composition it replaces; prints ONE JSON line (and writes it to profiles/rank_bench.json with --out).

Table: N = 2.5 M rows x F = 128 fp32 (1.28 GB, the papers100M-shaped table of bench_kge.py scaled to one device), CONTINUOUS;
B = 64 and 1024 queries; the three measures; no filter block (its pass is B x degree lanes, not the sweep).

Baseline, not the code under test: per chunk of `--chunk` rows, table.gather(ids) into [chunk, F], then query @ rows.T (dot),
-cdist(p=1) (l1) or -cdist(p=2)^2 (l2), compare with the target's score and sum; the chunk keeps the [B, chunk] matrix at
B x chunk x 4 bytes (for cdist it is cut to B x chunk < 2^24, the largest grid its kernel launches with). The baseline's arithmetic is not the contract's (matmul order, fused multiply-adds), so its counts may
differ in ties; the script checks that they agree within 0.1 % of N and does not compare bits.

Per case, the median of `--reps` calls after `--warmup`, device events around the call (bench_sage_agg.timed). Reported:
  table_GBps   N F 4 ceil(B / 64) bytes over the time: what the sweep asks of L2 / HBM (a query tile reads the table once)
  Gstep_per_s  B N F per-column steps over the time
  valu_frac    steps x VALU operations per step (dot 2: mul, add; l1 2: sub, add |.|; l2 3: sub, mul, add) over the time, as a
               fraction of 78.6e12 fp32 VALU operations per second: 256 CUs x 4 SIMDs x 16 lanes x 2 (packed fp32) x 2.4 GHz,
               half the 157.3 TFLOP/s of the public specification because the contract forbids the fused multiply-add."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import timed  # noqa: E402

VALU_PEAK = 256 * 4 * 16 * 2 * 2.4e9
OPS_PER_STEP = {"dot": 2, "l1": 2, "l2": 3}


def composite(table, query, target, measure, chunk):
    """(greater, equal) by gathers and [B, chunk] score matrices"""
    import torch
    n = table.shape[0]
    rows = table.gather(target)
    if measure == "dot":
        thr = (query * rows).sum(-1)
    elif measure == "l1":
        thr = -(query - rows).abs().sum(-1)
    else:
        thr = -(query - rows).pow(2).sum(-1)
    if measure != "dot":      # torch's cdist kernel runs a workgroup of 256 per output element: keep its grid below 2^32 lanes
        chunk = min(chunk, ((1 << 24) - 1) // query.shape[0])
    greater = torch.zeros(query.shape[0], dtype=torch.int64, device=query.device)
    equal = torch.zeros_like(greater)
    for s in range(0, n, chunk):
        ids = torch.arange(s, min(n, s + chunk), device=query.device)
        part = table.gather(ids)
        if measure == "dot":
            sc = query @ part.t()
        elif measure == "l1":
            sc = -torch.cdist(query, part, p=1.0)
        else:
            sc = -torch.cdist(query, part, p=2.0, compute_mode="donot_use_mm_for_euclid_dist").pow(2)
        own = ids[None, :] == target[:, None]
        greater += ((sc > thr[:, None]) & ~own).sum(1)
        equal += ((sc == thr[:, None]) & ~own).sum(1)
    return greater, equal


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--rows", type=int, default=2_500_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--queries", default="64,1024")
    p.add_argument("--measures", default="dot,l1,l2")
    p.add_argument("--chunk", type=int, default=262_144, help="rows per [B, chunk] score matrix of the baseline")
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_rank.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.wholegraph_ops import RANK_QUERY_TILE, rank_rows
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)

    N, F = a.rows, a.dim
    gen = torch.Generator(device="cuda").manual_seed(4)
    table = wgth.create_wholememory_tensor(comm, "continuous", "cuda", [N, F], torch.float32, None)
    table.get_local_tensor()[0].copy_(torch.randn((N, F), device="cuda", generator=gen))
    results = []
    for B in (int(v) for v in a.queries.split(",")):
        query = torch.randn((B, F), device="cuda", generator=gen)
        target = torch.randint(0, N, (B,), device="cuda", generator=gen)
        for measure in a.measures.split(","):
            ms = timed(lambda: rank_rows(table, query, target, measure=measure), a.warmup, a.reps)
            base_ms = timed(lambda: composite(table, query, target, measure, a.chunk), 1, max(2, a.reps // 2))
            g, e = rank_rows(table, query, target, measure=measure)
            cg, ce = composite(table, query, target, measure, a.chunk)
            worst = int(((g + e) - (cg + ce)).abs().max())
            assert worst <= N // 1000, "the baseline counts something else: %d rows apart" % worst
            steps = B * N * F
            passes = -(-B // RANK_QUERY_TILE)
            results.append({"queries": B, "measure": measure, "rows": N, "dim": F, "ms": round(ms, 4),
                            "table_GBps": round(N * F * 4 * passes / ms / 1e6, 1), "Gstep_per_s": round(steps / ms / 1e6, 1),
                            "valu_frac": round(steps * OPS_PER_STEP[measure] / (ms * 1e-3) / VALU_PEAK, 4),
                            "torch_ms": round(base_ms, 4), "speedup_vs_torch": round(base_ms / ms, 2),
                            "max_count_difference_vs_torch": worst})
            print(results[-1], file=sys.stderr, flush=True)
    line = {"bench": "rank_rows", "query_tile": RANK_QUERY_TILE, "valu_peak_ops": VALU_PEAK, "baseline_chunk": a.chunk,
            "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
