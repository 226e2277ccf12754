"""bench.py prints exactly one JSON line with the contract keys — at N = 1, and through the N > 1 code path (bucketing,
exchange, checks, max-over-ranks timing, the `exchange` object), which the test boxes can only run with several ranks on
ONE GPU and host collectives (`--backend gloo`; RCCL refuses two ranks on a device)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CONTRACT = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"]


def _one_json_line(stdout):
    lines = [x for x in stdout.decode().splitlines() if x.strip()]
    assert len(lines) == 1, "stdout must carry exactly the JSON record:\n" + stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_single_gpu_line(wm_lib):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--rows", "4000000", "--indices", "500000",
                        "--steps", "3", "--warmup", "1", "--cpu-seconds", "0.5"], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = _one_json_line(p.stdout)
    assert all(k in r for k in CONTRACT) and r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1
    assert r["unit"] == "GB/s" and r["higher_is_better"] is True and r["vs_baseline"] is None and r["dtype"] == "f32"
    assert "workload" in r["config"] and r["value"] > 0 and r["ms_per_step"] > 0
    roof = r["roofline"]
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert roof["algorithmic_bytes_per_launch"] == 500000 * (8 + 512 + 512)
    assert "rows_batch_kernel" in roof["kernel"]                # (the in-order kernel of 512 B rows) the name comes from the HIP runtime, not from bench.py
    # what each time in the object is (round-4 review): the HIP-event time of a step, the rocprofv3 average of the kernel when
    # profiles/ holds one for this workload (not for this toy size), and the same launch as a sequential copy in this process
    assert roof["step_ms_hip_events"] > 0 and "kernel_ms" not in roof and "kernel_ms_rocprof" in roof and "kernel_ms_source" in roof
    # one box per number (round-5 review): a kernel time cited for THIS line never exceeds this line's step
    if roof["kernel_ms_rocprof"] is not None:
        assert roof["kernel_ms_rocprof"] <= r["ms_per_step"] and abs(roof["profile_step_ms"] - r["ms_per_step"]) <= 0.02 * r["ms_per_step"]
    assert roof["copy_ms_sequential_ids"] > 0 and 0 < roof["copy_frac"] < 1
    assert abs(roof["vs_copy"] - roof["copy_ms_sequential_ids"] / roof["step_ms_hip_events"]) < 1e-2
    cpu = r["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and "sample" in cpu
    assert cpu["c1_shape"]["value"] > 0 and "10000000x64" in cpu["c1_shape"]["sample"]
    assert r["gpu_c1_host"]["value"] > 0 and r["gpu_c1_host"]["bound"] == "pcie"
    st = r["stability"]
    assert st["steps"] == 200 and 0 < st["min_ms"] <= st["median_ms"] <= st["p95_ms"] <= st["max_ms"]
    assert r["transport"] == "none" and r["rccl_ranks"] == 0


def test_plain_line_times_only_and_dumps_its_outputs(wm_lib, tmp_path):
    """Without --full the line carries the headline figures and none of the side legs; --dump-outputs writes a fixed, seeded
    sample of the last step's gathered rows (float32), the same bytes from one process to the next."""
    dumps = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "4000000", "--indices", "500000",
                            "--steps", "4", "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        r = _one_json_line(p.stdout)
        assert all(k in r for k in CONTRACT) and r["steps"] == 4 and r["warmup"] == 1 and r["ms_per_step"] > 0
        assert r["unit"] == "GB/s" and r["higher_is_better"] is True and r["dtype"] == "f32" and r["value"] > 0
        for side in ("stability", "cpu_baseline", "gpu_c1_host", "gpu_c1_host_cached", "side_errors"):
            assert side not in r, side
        assert r["table_probe"] is None and "copy_ms_sequential_ids" not in r["roofline"]
        assert sorted(os.listdir(str(d))) == ["gather_out.npy"]
        dumps.append(np.load(str(d / "gather_out.npy")))
    got = dumps[0]
    assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 128 and 1000 < got.shape[0] < 500000
    assert got.nbytes <= 64 << 20
    # closed-form table: every gathered row holds one integral row id in all its columns
    assert np.all(got == got[:, :1]) and np.all(got[:, 0] == np.floor(got[:, 0])) and got.min() >= 0 and got.max() < 4000000
    assert got.tobytes() == dumps[1].tobytes()


def test_self_launch_without_a_launcher(wm_lib):
    """`python bench.py --gpus 2` with no RANK in the environment starts the ranks itself (reference bench:
    gather_scatter_bench.cu:257-284 forks one process per device)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--backend", "gloo", "--rows", "1000003",
                        "--indices", "300000", "--steps", "3", "--warmup", "1", "--stability-steps", "5"],
                       capture_output=True, timeout=900, env=dict(env, OMP_NUM_THREADS="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = _one_json_line(p.stdout)
    assert r["n_gpus"] == 2 and r["transport"] == "external" and r["rccl_ranks"] == 0 and r["stability"]["steps"] == 5


def test_eight_ranks_exchange_object(wm_lib):
    """The N = 8 plumbing of bench.py before the first SCALE run: 8 ranks (sharing the one GPU, host collectives), toy
    sizes, the line's `exchange` object with the bytes every ordered pair moves per step and the link-bound prediction."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "8", "--backend", "gloo", "--rows", "250007",
                        "--indices", "80000", "--steps", "2", "--warmup", "1", "--stability-steps", "0"],
                       capture_output=True, timeout=900, env=dict(env, OMP_NUM_THREADS="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = _one_json_line(p.stdout)
    assert all(k in r for k in CONTRACT) and r["n_gpus"] == 8 and r["scaling"] == "weak"
    assert "C3 distributed 2000056x128" in r["config"]["workload"] and r["config"]["rows_per_gpu"] == 250007
    ex = r["exchange"]
    assert ex["bound"] == "xgmi" and ex["link_peak_GBps_per_direction"] == 76.8
    assert ex["bytes_per_ordered_pair_per_step"] == 80000 / 8 * (512 + 8)        # rows + ids of one peer's share
    assert abs(ex["predicted_link_bound_ms_per_step"] - 80000 / 8 * 520 / 76.8e9 * 1e3) < 1e-3
    assert ex["predicted_link_bound_value_GBps"] > 0 and "BRING-UP" in ex["note"]
    assert r["roofline"]["bound"] == "hbm" and "owner-side row gather" in r["roofline"]["scope"]
    assert r["c3_zipf"]["dedup_auto_ms_per_step"] > 0 and r["c3_zipf"]["dedup_off_ms_per_step"] > 0
    assert "side_errors" not in r, r.get("side_errors")


def test_more_gpus_than_visible_fails_loudly(wm_lib):
    import torch
    n = torch.cuda.device_count() + 1
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1"],
                       capture_output=True, timeout=300)
    assert p.returncode != 0 and b"visible" in p.stderr and p.stdout.strip() == b""


def test_forced_rccl_single_rank_reports_its_transport(wm_lib):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "4000000", "--indices", "500000",
                        "--memory-type", "distributed", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                        "--stability-steps", "0"], capture_output=True, timeout=600,
                       env=dict(os.environ, WM_FORCE_RCCL="1", WM_EXCHANGE_SELF="1", WM_RCCL_SELF_SENDRECV="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = _one_json_line(p.stdout)
    assert r["transport"] == "rccl" and r["rccl_ranks"] == 1 and r["n_gpus"] == 1 and "stability" not in r


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_line_over_host_collectives(wm_lib, world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(world), "--backend", "gloo",
           "--rows", "1000003", "--indices", "300000", "--steps", "3", "--warmup", "1"]
    p = subprocess.run(cmd, capture_output=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = _one_json_line(p.stdout)
    assert all(k in r for k in CONTRACT) and r["n_gpus"] == world and r["scaling"] == "weak"
    assert r["config"]["memory_type"] == "distributed" and r["config"]["rows_per_gpu"] == 1000003
    assert r["value"] > 0 and "cpu_baseline" not in r            # the host baseline is an N = 1 item
    assert r["exchange"]["bound"] == "xgmi" and "BRING-UP" in r["exchange"]["note"]
    assert r["roofline"]["bound"] == "hbm" and r["roofline"]["achieved"] > 0 and "local shard" in r["roofline"]["scope"]
    assert r["c3_zipf"]["dedup_auto_ms_per_step"] > 0 and r["c3_zipf"]["dedup_off_ms_per_step"] > 0   # the Zipf side leg (C3)
    # whole-job aggregate: all ranks' lookups over the slowest rank's time
    assert abs(r["mlookups_per_s"] - world * 300000 / (r["ms_per_step"] * 1e-3) / 1e6) / r["mlookups_per_s"] < 0.02


@pytest.mark.parametrize("world", [1, 2])
def test_sample_gather_line(wm_lib, world, tmp_path):
    """BASELINE config 5 as a bench op (small graph): one JSON line with the contract keys and its own roofline object; at
    world 2 the CSR and the features are DISTRIBUTED over two ranks sharing the GPU (collectives over gloo). The last step's
    features and sub-graph node ids are dumped, every rank its own."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--op", "sample_gather", "--nodes", "2000003", "--avg-degree", "12",
           "--seeds", "512", "--fanouts", "10,5", "--steps", "3", "--warmup", "2", "--stability-steps", "4",
           "--dump-outputs", str(tmp_path)]
    if world > 1:
        cmd += ["--gpus", str(world), "--backend", "gloo"]
    p = subprocess.run(cmd, capture_output=True, timeout=900, env=dict(env, OMP_NUM_THREADS="1"))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = _one_json_line(p.stdout)
    assert all(k in r for k in CONTRACT) and r["n_gpus"] == world and r["unit"] == "GB/s" and r["value"] > 0
    assert r["config"]["fanouts"] == [10, 5] and r["frontier_sizes"][-1] == 512 and len(r["frontier_sizes"]) == 3
    assert r["frontier_sizes"][0] == r["subgraph_nodes_per_step"] > 512 and r["sampled_edges_per_step"] > 0
    roof = r["roofline"]
    assert roof["bound"] == "hbm" and "latency" in roof["limited_by"] and 0 < roof["frac"] < 1
    assert r["stability"]["steps"] == 4
    for rank in range(world):
        sfx = "_rank%d" % rank if rank else ""
        x, ids = np.load(str(tmp_path / ("sample_gather_features%s.npy" % sfx))), np.load(str(tmp_path / ("sample_gather_node_ids%s.npy" % sfx)))
        assert x.dtype == np.float32 and ids.dtype == np.float64 and x.shape == (ids.shape[0], 128) and ids.shape[0] > 512
        assert np.array_equal(x[:, 0], ids) and np.all(x == x[:, :1]) and ids.max() < 2000003     # closed-form features


@pytest.mark.parametrize("world", [2, 4])
def test_first_contact_kit_dry_run(wm_lib, world, tmp_path):
    """scripts/first_contact.sh — what runs first on a multi-GPU node — end to end at toy sizes over gloo (the ranks share this
    box's GPU): every leg produces its bench line (uniform / Zipf hashed / Zipf clustered at 2 ... N ranks, the CHUNKED table by
    direct peer loads and through the exchange, C4 in fp16 and fp32, C5) and the report holds them next to the predictions."""
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")},
               FIRST_CONTACT_DRY="1", FIRST_CONTACT_OUT=str(tmp_path), OMP_NUM_THREADS="1")
    p = subprocess.run(["bash", os.path.join(ROOT, "scripts", "first_contact.sh"), str(world)], capture_output=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stdout.decode()[-3000:] + p.stderr.decode()[-2000:]
    rep = json.load(open(os.path.join(str(tmp_path), "first_contact.json")))
    assert rep["dry_run"] is True and rep["failed_step"] is None and rep["ranks"] == world
    m = rep["measured"]
    want = ["chunked_direct_n%d" % world, "chunked_via_exchange_n%d" % world, "c4_grad_apply_f16_n%d" % world,
            "c4_grad_apply_f32_n%d" % world, "c5_sample_gather_n%d" % world]
    k = 2
    while k <= world:
        want += ["c3_uniform_n%d" % k, "c3_zipf_n%d" % k, "c3_zipf_clustered_n%d" % k]
        k *= 2
    for name in want:
        assert name in m and m[name].get("value", 0) > 0 and "side_errors" not in m[name], (name, m.get(name))
    assert m["c3_zipf_clustered_n%d" % world]["config"]["index_distribution"] == "zipf_clustered"
    assert m["chunked_direct_n%d" % world]["config"]["memory_type"] == "chunked"
    assert str(world) in rep["predictions_uniform"] and rep["predictions_uniform"]["2"]["link_bound_ms_at_76.8"] > 30


def test_committed_kernel_profile_is_consistent_with_its_own_collection():
    """profiles/kernel_ms.json (what bench.py may cite as roofline.kernel_ms_rocprof) carries the step time of the collection it
    was measured in, and inside that collection the kernel does not take longer than the step that contains it."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "kernel_ms.json")))
    assert rec["collection_ms_per_step"] > 0 and rec["average_ms"] <= rec["collection_ms_per_step"]
    assert os.path.exists(os.path.join(ROOT, "profiles", rec["file"]))
