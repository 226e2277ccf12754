"""Random walks on the MI355X (csrc/kernels/walk.hip through wholegraph_ops.random_walk / GraphStructure.random_walk)
against the definition restated in Python (tests/_walk_ref.py), bit for bit, `walks` and `edge_ids`.

The ladder graph (2000 nodes of up to 12 neighbours, nodes 7 .. 15 with 5000, 1024, 1025, 63, 64, 0, 1, 65 and 2, a fifth of
the edges redirected to those nine) puts rows around the weighted kernel's group size and far above it, a node without
neighbours and a node whose weights are all ineligible on the way of 512 walks, three of which start outside the graph; the
reference walks are computed once and shared, and lower bounds on them keep every case populated. Also: a damaged graph ends
walks instead of faulting, batches that are no multiple of a block, the independence of a walk from its batch, seeds, the
DISTRIBUTED answer, and the distribution of the picks on a star graph."""
import numpy as np
import pytest

import _walk_ref as ref

pytestmark = pytest.mark.gpu

NP_OF = {"int32": np.int32, "int64": np.int64}


def _wm_array(comm, mt, arr, loc="cuda"):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr), loc)        # (a writable copy: the shared arrays are read-only)


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm, mt, loc, col_dtype, weights=None):
    import wholegraph_amd.torch as wgth
    row_ptr, col, _, _ = ref.ladder()
    ts = [_wm_array(comm, mt, row_ptr, loc), _wm_array(comm, mt, col.astype(col_dtype), loc)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    if weights is not None:
        ts.append(_wm_array(comm, mt, weights, loc))
        g.set_edge_attribute("w", ts[2])
    return g, ts


def _assert_equal(got, want, col_dtype, what):
    import torch
    walks, eids = got
    assert walks.dtype == torch.from_numpy(np.empty(0, dtype=col_dtype)).dtype and eids.dtype == torch.int64, what
    assert tuple(walks.shape) == want[0].shape and tuple(eids.shape) == want[1].shape, what
    assert np.array_equal(walks.cpu().numpy(), want[0].astype(col_dtype)), "walks differ: %s" % what
    assert np.array_equal(eids.cpu().numpy(), want[1]), "edge ids differ: %s" % what


# ------------------------------------------------------------------------------------------------ uniform
@pytest.mark.parametrize("mt,loc", [("continuous", "cuda"), ("chunked", "cuda"), ("continuous", "cpu"), ("chunked", "cpu")])
@pytest.mark.parametrize("start_dtype,col_dtype", [("int64", "int64"), ("int32", "int32"), ("int64", "int32"), ("int32", "int64")])
def test_uniform_walks_equal_the_reference(gpu_env, mt, loc, start_dtype, col_dtype):
    import torch
    ref.assert_ladder_measures()
    starts = ref.ladder()[3]
    g, ts = _structure(gpu_env, mt, loc, NP_OF[col_dtype])
    dev_starts = torch.from_numpy(starts.astype(NP_OF[start_dtype])).cuda()
    for length in (1, 6, 33):
        got = g.random_walk(dev_starts, length, random_seed=ref.LADDER_SEED, need_edge_ids=True)
        _assert_equal(got, ref.ladder_uniform(length), NP_OF[col_dtype], "L = %d" % length)
        only = g.random_walk(dev_starts, length, random_seed=ref.LADDER_SEED)
        assert torch.equal(only, got[0]), "walks without edge ids, L = %d" % length
    _destroy(ts)


def test_uniform_walks_on_plain_device_tensors(gpu_env):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    row_ptr, col, _, starts = ref.ladder()
    hold = [torch.from_numpy(np.array(a)).cuda() for a in (row_ptr, col.astype(np.int32))]
    wr, wc = [wrap_torch_tensor(t) for t in hold]
    got = wops.random_walk(wr.handle, wc.handle, torch.from_numpy(np.array(starts)).cuda(), ref.LADDER_LENGTH, ref.LADDER_SEED,
                           need_edge_output=True)
    _assert_equal(got, ref.ladder_uniform(), np.int32, "plain device tensors")


# ------------------------------------------------------------------------------------------------ weighted
@pytest.mark.parametrize("wdtype", [np.float32, np.float64])
@pytest.mark.parametrize("mt", ["continuous", "chunked"])
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_weighted_walks_equal_the_reference(gpu_env, wdtype, mt, col_dtype):
    import torch
    u, w = ref.assert_ladder_measures()
    _, _, weights, starts = ref.ladder()
    g, ts = _structure(gpu_env, mt, "cuda", NP_OF[col_dtype], weights.astype(wdtype))     # (double: the float ones widened)
    dev_starts = torch.from_numpy(np.array(starts)).cuda()
    got = g.random_walk(dev_starts, ref.LADDER_LENGTH, weight_name="w", random_seed=ref.LADDER_SEED, need_edge_ids=True)
    _assert_equal(got, ref.ladder_weighted(), NP_OF[col_dtype], "weighted")
    taken = got[1][got[1] >= 0].cpu().numpy()
    assert (weights[taken] > 0).all(), "a step over an edge whose weight is not positive"
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ a damaged graph
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_damaged_col_ind_ends_walks(gpu_env, col_dtype):
    """col_ind entries of -1, n_nodes and 2^31 - 1: the walk that picks one ends there, -1 in both outputs, and the call
    succeeds; every id that IS written indexes row_ptr"""
    import torch
    import wholegraph_amd.torch as wgth
    row_ptr, col, weights, starts = ref.ladder()
    bad = np.array(col)
    hit = np.arange(3, bad.shape[0], 7)
    bad[hit] = np.array([-1, ref.LADDER_NODES, (1 << 31) - 1], dtype=np.int64)[np.arange(hit.shape[0]) % 3]
    ts = [_wm_array(gpu_env, "chunked", a) for a in (row_ptr, bad.astype(NP_OF[col_dtype]), weights)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("w", ts[2])
    dev_starts = torch.from_numpy(np.array(starts)).cuda()
    u_want = ref.uniform_walks(row_ptr, bad, starts, ref.LADDER_LENGTH, ref.LADDER_SEED)
    assert ((u_want[0][:, 1:] < 0) & (u_want[0][:, :-1] >= 0)).sum() >= 100, "too few walks meet a damaged entry"
    got = g.random_walk(dev_starts, ref.LADDER_LENGTH, random_seed=ref.LADDER_SEED, need_edge_ids=True)
    torch.cuda.synchronize()
    _assert_equal(got, u_want, NP_OF[col_dtype], "uniform, damaged")
    walks, eids = g.random_walk(dev_starts, ref.LADDER_LENGTH, weight_name="w", random_seed=ref.LADDER_SEED, need_edge_ids=True)
    torch.cuda.synchronize()
    walks, eids = walks.cpu().numpy().astype(np.int64), eids.cpu().numpy()
    assert ((walks >= 0) & (walks < ref.LADDER_NODES) | (walks == -1)).all()
    ended = walks[:, 1:] < 0
    assert np.array_equal(ended, eids < 0) and (np.diff(ended.astype(np.int8), axis=1) >= 0).all(), "-1 from the end on, in both"
    assert np.array_equal(bad[eids[~ended]], walks[:, 1:][~ended])
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ edge cases
def test_empty_batch_batch_independence_and_seeds(gpu_env):
    import torch
    starts = ref.ladder()[3]
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, ref.ladder()[2])
    dev_starts = torch.from_numpy(np.array(starts)).cuda()
    for name in (None, "w"):
        walks, eids = g.random_walk(dev_starts[:0], 4, weight_name=name, random_seed=5, need_edge_ids=True)
        assert tuple(walks.shape) == (0, 5) and tuple(eids.shape) == (0, 4) and walks.dtype == torch.int64
        whole = g.random_walk(dev_starts, ref.LADDER_LENGTH, weight_name=name, random_seed=ref.LADDER_SEED, need_edge_ids=True)
        first = g.random_walk(dev_starts[:100], ref.LADDER_LENGTH, weight_name=name, random_seed=ref.LADDER_SEED, need_edge_ids=True)
        assert torch.equal(whole[0][:100], first[0]) and torch.equal(whole[1][:100], first[1]), "a walk depends on its batch"
        again = g.random_walk(dev_starts, ref.LADDER_LENGTH, weight_name=name, random_seed=ref.LADDER_SEED, need_edge_ids=True)
        assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1]), "the same seed, other walks"
        a = g.random_walk(dev_starts, ref.LADDER_LENGTH, weight_name=name)
        b = g.random_walk(dev_starts, ref.LADDER_LENGTH, weight_name=name)
        assert not torch.equal(a, b), "no seed given twice: the same walks"
    _destroy(ts)


def test_many_uniform_walks_equal_the_reference(gpu_env):
    """70001 walks of 4 steps: no multiple of any block size, more than one block per CU"""
    import torch
    row_ptr, col, _, _ = ref.ladder()
    n = 70001
    starts = np.random.default_rng(17).integers(-2, ref.LADDER_NODES + 2, n).astype(np.int32)
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int32)
    got = g.random_walk(torch.from_numpy(starts).cuda(), 4, random_seed=31, need_edge_ids=True)
    _assert_equal(got, ref.uniform_walks(row_ptr, col, starts, 4, 31), np.int32, "70001 walks")
    _destroy(ts)


def test_distributed_csr_is_not_implemented(gpu_env):
    import torch
    from wholegraph_amd import binding
    row_ptr, col, weights, starts = ref.ladder()
    dev_starts = torch.from_numpy(np.array(starts)).cuda()
    g, ts = _structure(gpu_env, "distributed", "cuda", np.int64)
    with pytest.raises(binding.WholeMemoryError) as e:
        g.random_walk(dev_starts, 3, random_seed=1)
    assert e.value.code == 2 and isinstance(e.value, NotImplementedError)      # WHOLEMEMORY_NOT_IMPLEMENTED
    _destroy(ts)
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64)
    ts.append(_wm_array(gpu_env, "distributed", weights))
    g.set_edge_attribute("w", ts[2])
    with pytest.raises(binding.WholeMemoryError) as e:
        g.random_walk(dev_starts, 3, weight_name="w", random_seed=1)
    assert e.value.code == 2
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_picks_on_a_star_follow_the_weights_and_are_independent(gpu_env, weighted):
    """8000 walks of 5 steps from the centre of a star with 8 leaves (weights 1 .. 8): columns 2 and 4 are the centre again;
    columns 1, 3 and 5 fit the expected counts (chi-square over 7 degrees of freedom below 40, the bar of
    tests/test_sampler_edges_gpu.py, p ~ 1e-6) and the 8 x 8 tables of columns (1, 3), (3, 5) and of walks w against w + s, s in
    1, 2, 64, 1024, stay below 110 over 49 degrees of freedom (about six standard deviations)."""
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    row_ptr, col, weights = ref.star()
    hold = [torch.from_numpy(a).cuda() for a in (row_ptr, col, weights)]
    wr, wc, ww = [wrap_torch_tensor(t) for t in hold]
    starts = torch.zeros(ref.STAR_WALKS, dtype=torch.int64, device="cuda")
    walks = wops.random_walk(wr.handle, wc.handle, starts, ref.STAR_LENGTH, ref.STAR_SEED,
                             wm_csr_weight_ptr_tensor=ww.handle if weighted else None)
    fit, independence = ref.star_statistics(walks.cpu().numpy(), weighted)
    print("star, %s: goodness of fit %.2f over 7 dof, independence %.2f over 49 dof" % (
        "weighted" if weighted else "uniform", fit, independence))
    assert fit < 40.0, "chi-square %.1f over 7 dof" % fit
    assert independence < 110.0, "chi-square %.1f over 49 dof" % independence
