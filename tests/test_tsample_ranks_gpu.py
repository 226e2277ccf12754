"""The temporal sampler on a graph that lives on 2 ranks (MI355X; both ranks share cuda:0), after
tests/test_csr_graph_ranks_gpu.py: the temporal ladder split in equal chunks, in a custom partition that cuts csr_row_ptr
between s and e of the hub and cuts col_ind AND the edge times inside the hub's row, and DISTRIBUTED, where the Python op
composes the route. Every rank asks for a batch of its own, exact against the single-rank reference fed the full arrays
(tests/_tsample_ref.py); the worker (tests/_tsample_ranks_worker.py) states the layouts and what each rank passes. The launch
runs under its own timeout and a failed rank ends the other. Also, on one rank, a DISTRIBUTED graph gives the reference's
samples (tests/test_tsample_gpu.py holds that case: test_distributed_tensors_give_the_reference_samples)."""
import os
import subprocess
import sys
import tempfile
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 2
TIMEOUT = 120          # seconds: a safety net, the launch takes a fraction of it
_LAUNCH = []


def launch():
    """-> [(return code, output) per rank] of the worker job, run once. A rank that fails ends the other: it would wait for
    it in a collective until the timeout."""
    if not _LAUNCH:
        from test_distributed_cpu import free_port
        port = str(free_port())
        env = dict(os.environ, OMP_NUM_THREADS="1")
        logs = [tempfile.TemporaryFile() for _ in range(WORLD)]
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_tsample_ranks_worker.py"), str(r), str(WORLD), port],
                                  env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(WORLD)]
        deadline = time.monotonic() + TIMEOUT
        try:
            while any(p.poll() is None for p in procs):
                if time.monotonic() > deadline or any(p.returncode not in (None, 0) for p in procs):
                    break
                try:
                    next(p for p in procs if p.returncode is None).wait(timeout=0.2)
                except subprocess.TimeoutExpired:
                    pass
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                p.wait()
        for p, log in zip(procs, logs):
            log.seek(0)
            _LAUNCH.append((p.returncode, log.read().decode(errors="replace")))
            log.close()
    return _LAUNCH


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["chunked", "custom", "distributed"])
def test_temporal_sampler_on_a_graph_split_over_two_ranks(wm_lib, layout):
    ranks = launch()
    for r, (code, out) in enumerate(ranks):
        tails = "\n=====\n".join(o[-2500:] for _, o in ranks)
        assert code == 0 and ("RANK %d OK" % r) in out, "rank %d failed:\n%s" % (r, tails)
        assert ("RANK %d %s OK" % (r, layout)) in out, "rank %d did not finish %s:\n%s" % (r, layout, tails)


def test_the_cuts_fall_inside_the_hub_row():
    """the partition arrays alone (no GPU): a later change of the ladder cannot silently move a cut to a row boundary"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _tsample_ranks_worker as worker
    import _tsample_ref as ref
    row_ptr = ref.temporal_ladder()[0]
    p = worker.custom_partitions(WORLD)
    assert p["row"][0] == worker.HUB + 1 and row_ptr[worker.HUB] < p["edge"][0] < row_ptr[worker.HUB + 1]
    assert p["row"][0] < p["row"][1] and p["edge"][0] < p["edge"][1]      # (the first partition is the smaller: a search)
    for rank in range(WORLD):
        assert worker.HUB in worker.rank_batch(rank)[0].tolist()
