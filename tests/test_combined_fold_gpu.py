"""The sender-side fold of duplicate gradient rows (embedding.cpp: combined_gradient_apply; not in the reference, which ships every
copy: embedding.cpp:193-247) on batches whose distinct ids are nearly all LONG runs, and the automatic decision that selects the
route (tests/_dist_worker.py: scenario_combined_dense, scenario_combine_auto; WM_TEST_ONLY=combined_dense runs these alone).

The tree fold lists a run by its ROWS: a sender whose 64 distinct ids have 129 ... 1100 copies each lists 64 runs, and the
workspace they are listed in must be carved by the batch's rows, not by its 64 distinct ids. Every comparison is byte equality
with the ordered multi-rank oracle (integer-valued gradients with small partial sums: any association order gives the same bits),
so a dropped, doubled or misplaced row shows.

The fp32 legs also run over gloo on the CPU test backend (its duplicate estimate is exact, its fold the ordered one): that pins
the orchestration, the vote in the counts exchange and the scenarios' own premise without a GPU. The 16-bit tables, the mapped
table types and the tree kernels themselves need the HIP backend."""
import os
import subprocess

import pytest

from test_distributed_cpu import ROOT, run_world

ONLY = {"WM_TEST_ONLY": "combined_dense"}


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "3"])
@pytest.mark.parametrize("world", [2, 3])
def test_combined_dense_hip_kernels(wm_lib, world, chunks):
    """`world` processes sharing cuda:0 (at most three hold the GPU), collectives over gloo"""
    run_world(world, "hip", dict(ONLY, WM_EXCHANGE_CHUNKS=chunks))


@pytest.mark.gpu
def test_combined_dense_rccl_loopback(wm_lib):
    """one rank whose own segment travels through the RCCL transport like a peer's: the combined route is taken at world 1"""
    run_world(1, "hip-rccl", dict(ONLY, WM_FORCE_RCCL="1", WM_EXCHANGE_SELF="1", WM_RCCL_SELF_SENDRECV="1"))


@pytest.mark.parametrize("world", [2, 3])
def test_combined_dense_over_gloo(wm_lib, world):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "test_backend"], stdout=subprocess.DEVNULL)
    run_world(world, "cpu", dict(ONLY, WHOLEGRAPH_AMD_TESTING="1", HIP_VISIBLE_DEVICES="", WM_EXCHANGE_CHUNKS="1"))
