#!/usr/bin/env python3
"""Timing of `gather_agg_concat` over an 8-bit row-quantized table (wholegraph_amd/torch/gather_aggregation.py ->
csrc/kernels/agg_quant.hip, header section 2j) against the two ops it replaces and against the fp32-table op, on one MI355X.

The block is layer 0 (the outermost block) of a BASELINE config 5 sample: 1024 seeds, fan-outs 30,30, on a graph built the
way bench.py --op sample_gather builds it (scripts/bench_gather_agg.py: c5_layer0), with as many nodes as the table has rows;
the node ids are the sampler's. The table is CHUNKED on the device, --table-rows x --dim (default 100 M x 128; halved until
the fp32 table fits in 70 % of the free device memory, every leg then uses that size).

Three legs, each timed in a process of its own (--runs processes per leg, one after the other; a leg's process builds the
graph, its own table and nothing else), median of --reps calls after --warmup, device events around whole calls:
  fused        gather_agg_concat(qtable, ids, ...)                the kernel that dequantizes the rows as it adds them
  composition  agg_concat(qtable.gather(ids), ...)                the two ops that exist without it: the baseline
  fp32         gather_agg_concat(fp32 table, ids, ...)            kernels/agg_gather.hip on a table four times the size
The fused and composition legs check first that the two results are equal bit for bit.
Bytes per call, R = round_up(dim, 4) + 8 (a quantized row), I = bytes of a node id, F = dim:
  algorithmic   fused: E (4 + I + R) + n_dst (4 + I + R + 8 F);  fp32: E (4 + I + 4 F) + n_dst (4 + I + 12 F)
                composition: n_src (I + R + 4 F) + E (4 + 4 F) + n_dst (4 + 12 F)
  fetched       the same with every row read counted as the whole --line-bytes lines it touches, from the rows' real
                offsets (a 136-byte row at a 144-byte stride always touches two 128-byte lines)
The report (--out) holds one line per process, then per leg the median over the runs and their spread (max / min of the
run medians), then the verdict: the fused leg counts as faster only when its slowest run beats the composition's fastest."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LEGS = ("fused", "composition", "fp32")


def fill_quantized(wgth, comm, rows, dim, row_align):
    import torch
    t = wgth.create_quantized_tensor(comm, "chunked", "cuda", [rows, dim], row_align=row_align)
    gen = torch.Generator(device="cuda").manual_seed(5)
    step = max(1, (1 << 26) // dim)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        t.scatter(torch.randn((r1 - r0, dim), device="cuda", generator=gen), torch.arange(r0, r1, device="cuda"))
    torch.cuda.synchronize()
    return t


def lines_touched(ids, stride, row_bytes, line):
    """mean number of `line`-byte lines a read of row_bytes at offset id * stride touches, over ids (a device tensor)"""
    off = ids.to("cuda").long() * stride
    return float((((off + row_bytes - 1) // line) - (off // line) + 1).double().mean())


def run_leg(a):
    import torch
    assert torch.cuda.is_available(), "bench_qagg.py measures the GPU: no GPU found"
    torch.cuda.set_device(0)
    from wholegraph_amd import binding
    import wholegraph_amd.torch as wgth
    from bench_gather_agg import c5_layer0, make_table
    from bench_sage_agg import timed_all
    from wholegraph_amd.torch import gather_aggregation
    from wholegraph_amd.torch.aggregation import agg_concat
    binding.check(binding.lib().wholememory_init(0, binding.LEVEL_WARN))
    comm = wgth.create_group_communicator(1)
    rows, dim = a.table_rows, a.dim
    row_ptr, col_ind, ids = c5_layer0(wgth, comm, rows, 29, a.seeds, [int(f) for f in a.fanouts.split(",")])
    n_dst, E, n_src = row_ptr.numel() - 1, col_ind.numel(), ids.numel()
    I, R, F = ids.element_size(), (dim + 3) // 4 * 4 + 8, dim
    if a.leg == "fp32":
        table = make_table(wgth, comm, rows, dim, torch.float32)
        stride = dim * 4

        def fn():
            return wgth.gather_agg_concat(table, ids, row_ptr, col_ind, "mean")
        before = gather_aggregation.calls()
        fn()
        assert gather_aggregation.calls() == before + 1, "the fp32 table-reading kernel did not run"
    else:
        table = fill_quantized(wgth, comm, rows, dim, a.row_align)
        stride = table.storage.stride()[0]

        def fused():
            return wgth.gather_agg_concat(table, ids, row_ptr, col_ind, "mean")

        def composition():
            return agg_concat(table.gather(ids), row_ptr, col_ind, "mean")
        before = gather_aggregation.quantized_calls()
        x, y = fused(), composition()
        ran = gather_aggregation.quantized_calls() - before
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "fused and composition results differ"
        del x, y
        fn = fused if a.leg == "fused" else composition
        if a.leg == "fused" and ran != 1:   # (gather_agg_concat routes quantized sources to the composition: time the kernel)
            import ctypes as C
            from wholegraph_amd.torch.wholegraph_env import get_stream, get_wholegraph_env_fns

            def fn():
                out = torch.empty((n_dst, 2 * dim), dtype=torch.float32, device="cuda")
                binding.check(binding.lib().wholememory_ext_csc_gather_dequantize_aggregate_forward(
                    table.storage.wmb_tensor, dim, C.c_void_p(ids.data_ptr()),
                    binding.DT_INT64 if I == 8 else binding.DT_INT, C.c_void_p(row_ptr.data_ptr()),
                    C.c_void_p(col_ind.data_ptr()), E, n_dst, n_src, binding.AGGR_MEAN, C.c_void_p(out.data_ptr()), 2 * dim,
                    get_wholegraph_env_fns(), C.c_void_p(get_stream())))
                return out
            before = gather_aggregation.quantized_calls()
            assert torch.equal(fn().view(torch.int32), composition().view(torch.int32))
            assert gather_aggregation.quantized_calls() == before + 1, "the fused kernel did not run"
    ms = timed_all(fn, a.warmup, a.reps)
    row_b = 4 * F if a.leg == "fp32" else R
    edge_ids = ids[col_ind.long()]
    per_edge = lines_touched(edge_ids, stride, row_b, a.line_bytes) * a.line_bytes
    per_self = lines_touched(ids[:n_dst], stride, row_b, a.line_bytes) * a.line_bytes
    per_src = lines_touched(ids, stride, row_b, a.line_bytes) * a.line_bytes
    if a.leg == "composition":
        algorithmic = n_src * (I + R + 4 * F) + E * (4 + 4 * F) + n_dst * (4 + 12 * F)
        fetched = n_src * (I + per_src + 4 * F) + E * (4 + 4 * F) + n_dst * (4 + 12 * F)   # (the fp32 rows are whole lines)
    else:
        algorithmic = E * (4 + I + row_b) + n_dst * (4 + I + row_b + 8 * F)
        fetched = E * (4 + I + per_edge) + n_dst * (4 + I + per_self + 8 * F)
    med = statistics.median(ms)
    print(json.dumps({"leg": a.leg, "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                      "n_dst": n_dst, "n_src": n_src, "edges": E, "dim": dim, "table_rows": rows, "row_stride_bytes": stride,
                      "row_bytes": row_b, "id_bytes": I, "algorithmic_bytes": int(algorithmic), "fetched_bytes": int(fetched),
                      "algorithmic_GBps": round(algorithmic / med / 1e6, 1), "fetched_GBps": round(fetched / med / 1e6, 1),
                      "routed_to_fused_kernel_by_default": bool(a.leg == "fused" and ran == 1) if a.leg != "fp32" else None,
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--runs", type=int, default=3, help="processes per leg")
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--table-rows", type=int, default=100_000_000)
    p.add_argument("--seeds", type=int, default=1024)
    p.add_argument("--fanouts", default="30,30")
    p.add_argument("--row-align", type=int, default=16)
    p.add_argument("--line-bytes", type=int, default=128)
    p.add_argument("--legs", default=",".join(LEGS))
    p.add_argument("--leg", choices=LEGS, help="(internal) run this one leg in this process and print its JSON line")
    p.add_argument("--leg-timeout", type=int, default=420, help="seconds a leg's process may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "qagg_bench.txt"))
    a = p.parse_args()
    if a.leg:
        return run_leg(a)

    # the parent never touches the GPU; the fp32 table decides the size every leg uses
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.mem_get_info()[0])"], capture_output=True,
                           text=True, timeout=a.leg_timeout, check=True)
    free, rows = int(probe.stdout.split()[-1]), a.table_rows
    while rows * a.dim * 4 > 0.7 * free and rows > 1_000_000:
        rows //= 2
    lines, by_leg = [], {}
    for run in range(a.runs):
        for leg in a.legs.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--warmup", str(a.warmup), "--reps", str(a.reps),
                   "--dim", str(a.dim), "--table-rows", str(rows), "--seeds", str(a.seeds), "--fanouts", a.fanouts,
                   "--row-align", str(a.row_align), "--line-bytes", str(a.line_bytes)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            if r.returncode != 0:   # (nothing more is started on the GPU behind a leg that failed)
                sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
                sys.exit("leg %s failed with exit status %d" % (leg, r.returncode))
            rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            rec["run"] = run
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            by_leg.setdefault(leg, []).append(rec)
    head = ("scripts/bench_qagg.py: layer 0 of a C5 sample (%d seeds, fan-outs %s), dim %d, CHUNKED device table of %d rows "
            "(asked: %d), %d processes per leg, warmup %d, median of %d calls each; times are whole calls in ms"
            % (a.seeds, a.fanouts, a.dim, rows, a.table_rows, a.runs, a.warmup, a.reps))
    summary = []
    for leg, recs in by_leg.items():
        meds = [r["median_ms"] for r in recs]
        m = statistics.median(meds)
        summary.append("%-12s run medians %s  median %.4f  spread max/min %.3f  algorithmic %.1f MB (%.0f GB/s)  fetched "
                       "(%d-byte lines) %.1f MB (%.0f GB/s)"
                       % (leg, " ".join("%.4f" % v for v in meds), m, max(meds) / min(meds), recs[0]["algorithmic_bytes"] / 1e6,
                          recs[0]["algorithmic_bytes"] / m / 1e6, a.line_bytes, recs[0]["fetched_bytes"] / 1e6,
                          recs[0]["fetched_bytes"] / m / 1e6))
    if "fused" in by_leg and "composition" in by_leg:
        f = [r["median_ms"] for r in by_leg["fused"]]
        c = [r["median_ms"] for r in by_leg["composition"]]
        summary.append("fused / composition = %.3f (medians); fused slowest %.4f vs composition fastest %.4f: the fused kernel "
                       "is %s beyond the run-to-run spread" % (statistics.median(f) / statistics.median(c), max(f), min(c),
                                                               "faster" if max(f) < min(c) else "NOT faster"))
    if "fused" in by_leg and "fp32" in by_leg:
        summary.append("fused / fp32 table = %.3f (medians)" % (statistics.median([r["median_ms"] for r in by_leg["fused"]]) /
                                                                statistics.median([r["median_ms"] for r in by_leg["fp32"]])))
    text = "\n".join([head] + lines + summary) + "\n"
    print("\n".join(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
