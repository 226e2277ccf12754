#!/usr/bin/env python3
"""Timing of the gather of an 8-bit row-quantized table (wholegraph_amd/torch/quantized.py -> csrc/kernels/qrows.hip) against
the fp32 gather it replaces and against the two ops one would compose without it, on one MI355X; prints ONE JSON line.

Two tables, each as an fp32 WholeMemory tensor and as a quantized one holding the same rows, in one process:
  device  CHUNKED on the device, 10 M x 128
  host    CHUNKED in host memory, 10 M x 64 (BASELINE config C1: the rows cross PCIe)
Per table and id count (1 M and 10 M uniform int64 ids), median of --reps calls after --warmup, device events:
  fp32        table.gather(ids)                                   float32 out
  fused_f32   qtable.gather(ids)                                  gather + dequantize in one call, float32 out (the entry
                                                                  point's own route; reported per result)
  fused_f16   qtable.gather(ids, force_dtype=float16)
  two_op      dequantize_rows(qtable.storage.gather(ids), dim)    int8 gather, then a pass over [n, row_bytes]
The fused result is checked against the two-op result bit for bit first. Algorithmic bytes per lookup, I = 8 (the id),
F = dim, R = quantized_row_bytes(F):
  fp32 I + 4F + 4F;  fused I + R + 4F (2F for float16);  two_op (I + R + R) + (R + 4F)
No threshold: the numbers are reported, "fused_beats_both" says whether the fused float32 median is below both others."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def make_tables(wgth, comm, location, rows, dim):
    """(fp32 tensor, quantized tensor) with the same N(0, 1) rows"""
    import torch
    plain = wgth.create_wholememory_tensor(comm, "chunked", location, [rows, dim], torch.float32, None)
    q = wgth.create_quantized_tensor(comm, "chunked", location, [rows, dim])
    gen = torch.Generator(device="cuda").manual_seed(5)
    step = max(1, (1 << 27) // dim)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        block = torch.randn((r1 - r0, dim), device="cuda", generator=gen)
        ids = torch.arange(r0, r1, dtype=torch.int64, device="cuda")
        plain.scatter(block, ids)
        q.scatter(block, ids)
    torch.cuda.synchronize()
    return plain, q


def run(name, plain, q, ids, dim, warmup, reps):
    import torch
    import wholegraph_amd.torch as wgth
    from bench_sage_agg import timed_all
    from wholegraph_amd.torch import quantized
    n, I, R = ids.numel(), ids.element_size(), wgth.quantized_row_bytes(dim)

    def two_op():
        return wgth.dequantize_rows(q.storage.gather(ids), dim)
    variants = {
        "fp32": (lambda: plain.gather(ids), I + 8 * dim),
        "fused_f32": (lambda: q.gather(ids), I + R + 4 * dim),
        "fused_f16": (lambda: q.gather(ids, force_dtype=torch.float16), I + R + 2 * dim),
        "two_op": (two_op, I + 3 * R + 4 * dim),
    }
    before = quantized.calls()
    a = variants["fused_f32"][0]()
    table_reading = quantized.calls() == before + 1   # (False: the entry point took its two steps, as for large host batches)
    b = two_op()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "fused and two-op results differ"
    del a, b
    res = {"table": name, "n_ids": n, "dim": dim, "row_bytes": R, "fused_is_table_reading_kernel": table_reading}
    for key, (fn, per_lookup) in list(variants.items()) + [("fused_f32_second_pass", variants["fused_f32"])]:
        ms = timed_all(fn, warmup, reps)
        med = statistics.median(ms)
        res[key] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                    "lookups_per_s": round(n / med * 1e3), "bytes_per_lookup": per_lookup,
                    "algorithmic_GBps": round(n * per_lookup / med / 1e6, 1)}
        torch.cuda.empty_cache()
    f = res["fused_f32"]["median_ms"]
    res["fused_over_fp32"] = round(f / res["fp32"]["median_ms"], 3)
    res["fused_over_two_op"] = round(f / res["two_op"]["median_ms"], 3)
    res["fused_beats_both"] = bool(f < res["fp32"]["median_ms"] and f < res["two_op"]["median_ms"])
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--ids", default="1000000,10000000")
    p.add_argument("--tables", default="device,host")
    p.add_argument("--out", help="also write the JSON line to this file")
    a = p.parse_args()

    import torch
    assert torch.cuda.is_available(), "bench_qrows.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    gen = torch.Generator(device="cuda").manual_seed(2)
    results = []
    for name in a.tables.split(","):
        location, dim = {"device": ("cuda", 128), "host": ("cpu", 64)}[name]
        plain, q = make_tables(wgth, comm, location, a.rows, dim)
        for n in (int(v) for v in a.ids.split(",")):
            ids = torch.randint(0, a.rows, (n,), device="cuda", generator=gen, dtype=torch.int64)
            results.append(run(name, plain, q, ids, dim, a.warmup, a.reps))
        wgth.destroy_wholememory_tensor(plain)
        wgth.destroy_wholememory_tensor(q.storage)
        torch.cuda.empty_cache()
    line = {"bench": "qrows", "device": torch.cuda.get_device_name(0), "rows": a.rows, "warmup": a.warmup, "reps": a.reps,
            "results": results, "fused_beats_both_everywhere": bool(all(r["fused_beats_both"] for r in results))}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
