#!/usr/bin/env python3
"""Timing of topk_rows (wholegraph_amd/torch/wholegraph_ops.py -> csrc/kernels/topk.hip) on one MI355X against rank_rows at the
same shape in the same process, and against the torch composition it replaces; prints ONE JSON line (and writes it to
profiles/topk_bench.json with --out).

Table: bench_rank.py's, N = 2.5 M rows x F = 128 fp32 (1.28 GB), CONTINUOUS; B = 64 and 1024 queries; k = 10 and 64; the
three measures; no filter block.

Yardstick: rank_rows sweeps the same table with the same arithmetic and keeps two integers per query, so topk_ms / rank_ms is
what the selection costs (the running tops in LDS, two workgroups a CU, the rounds after each row tile, the merge of the
splits). The two are timed alternately, call by call, and the median of each is taken.

Baseline, not the code under test: per chunk of `--chunk` rows, table.gather(ids) into [chunk, F], the [B, chunk] scores of
bench_rank.composite (matmul / cdist), torch.topk of the chunk, and a torch.topk over the running top and the chunk's. Its
arithmetic is not the contract's, so near-ties may come out in another order: the script reports the share of the [B, k]
positions that hold the same id and requires 98 %."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_sage_agg import timed  # noqa: E402


def composite(table, query, k, measure, chunk):
    """(ids, scores) [B, k] by gathers, [B, chunk] score matrices and torch.topk"""
    import torch
    n = table.shape[0]
    if measure != "dot":      # (bench_rank.composite: cdist's grid)
        chunk = min(chunk, ((1 << 24) - 1) // query.shape[0])
    best = torch.full((query.shape[0], k), float("-inf"), device=query.device)
    best_ids = torch.full((query.shape[0], k), -1, dtype=torch.int64, device=query.device)
    for s in range(0, n, chunk):
        ids = torch.arange(s, min(n, s + chunk), device=query.device)
        part = table.gather(ids)
        if measure == "dot":
            sc = query @ part.t()
        elif measure == "l1":
            sc = -torch.cdist(query, part, p=1.0)
        else:
            sc = -torch.cdist(query, part, p=2.0, compute_mode="donot_use_mm_for_euclid_dist").pow(2)
        v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1)
        v, i = torch.cat([best, v], 1), torch.cat([best_ids, i + s], 1)
        best, pos = torch.topk(v, k, dim=1)
        best_ids = torch.gather(i, 1, pos)
    return best_ids, best


def alternating(fa, fb, warmup, reps):
    """median device ms of fa and of fb, a call of each in turn"""
    import torch
    for _ in range(warmup):
        fa(), fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for which, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[which].append(e0.elapsed_time(e1))
    return statistics.median(ms[0]), statistics.median(ms[1]), max(ms[0]) / min(ms[0])


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--rows", type=int, default=2_500_000)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--queries", default="64,1024")
    p.add_argument("--ks", default="10,64")
    p.add_argument("--measures", default="dot,l1,l2")
    p.add_argument("--chunk", type=int, default=262_144, help="rows per [B, chunk] score matrix of the baseline")
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_topk.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.wholegraph_ops import rank_rows, topk_rows
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
            for k in (int(v) for v in a.ks.split(",")):
                ms, rank_ms, spread = alternating(lambda: topk_rows(table, query, k, measure=measure),
                                                  lambda: rank_rows(table, query, target, measure=measure), a.warmup, a.reps)
                base_ms = timed(lambda: composite(table, query, k, measure, a.chunk), 1, max(2, a.reps // 3))
                ids, _ = topk_rows(table, query, k, measure=measure)
                agree = float((ids == composite(table, query, k, measure, a.chunk)[0]).double().mean())
                assert agree >= 0.98, "the baseline selects something else: %.4f of the positions agree" % agree
                results.append({"queries": B, "measure": measure, "k": k, "rows": N, "dim": F, "ms": round(ms, 4),
                                "max_over_min": round(spread, 3), "rank_rows_ms": round(rank_ms, 4),
                                "topk_over_rank": round(ms / rank_ms, 3), "Gstep_per_s": round(B * N * F / ms / 1e6, 1),
                                "torch_ms": round(base_ms, 4), "speedup_vs_torch": round(base_ms / ms, 2),
                                "id_agreement_vs_torch": round(agree, 5)})
                print(results[-1], file=sys.stderr, flush=True)
    line = {"bench": "topk_rows", "baseline_chunk": a.chunk, "reps": a.reps, "results": results}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
