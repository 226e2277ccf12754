"""node2vec (p, q) walks on the MI355X (csrc/kernels/walk_n2v.hip through wholegraph_ops.node2vec_walk /
GraphStructure.node2vec_walk) against the definition restated in Python (tests/_n2v_ref.py), bit for bit, `walks` and
`edge_ids`.

The clustered ladder (2000 nodes on a ring whose neighbours lie at ring distance <= 8, so that nearby nodes share neighbours;
nodes 7 .. 15 with 5000, 1024, 1025, 63, 64, 0, 1, 65 and 2 neighbours, a fifth of the entries redirected to those nine) puts
ways back, neighbours of the previous node and strangers into one row, rows around the group size and far above it, a node
without neighbours and a node without an eligible one on the way of 512 walks; every row is ascending, so both search routes
must agree on it. Its unsorted twin holds the same rows shuffled (heavy rows cut to 1025 entries) for the scanning route alone.
The reference walks are computed once and shared, and lower bounds on them (tests/test_n2v_streams.py checks them without a
GPU) keep every case populated. Also: p = q = 1 against random_walk, a damaged graph, a broken col_sorted promise, a batch that
is no multiple of a block, the independence of a walk from its batch, seeds, the DISTRIBUTED answer, and the distribution of
the second step on the kite."""
import numpy as np
import pytest

import _n2v_ref as ref

pytestmark = pytest.mark.gpu

NP_OF = {"int32": np.int32, "int64": np.int64}
WEIGHTS = (None, np.float32, np.float64)


def _wm_array(comm, mt, arr, loc="cuda"):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr), loc)        # (a writable copy: the shared arrays are read-only)


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm, mt, loc, col_dtype, graph, weights=()):
    """-> GraphStructure over graph's row_ptr and col_ind, with one edge attribute "w<i>" per array of `weights`"""
    import wholegraph_amd.torch as wgth
    ts = [_wm_array(comm, mt, graph[0], loc), _wm_array(comm, mt, np.asarray(graph[1]).astype(col_dtype), loc)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    for i, w in enumerate(weights):
        ts.append(_wm_array(comm, mt, w, loc))
        g.set_edge_attribute("w%d" % i, ts[-1])
    return g, ts


def _assert_equal(got, want, col_dtype, what):
    import torch
    walks, eids = got
    assert walks.dtype == torch.from_numpy(np.empty(0, dtype=col_dtype)).dtype and eids.dtype == torch.int64, what
    assert tuple(walks.shape) == want[0].shape and tuple(eids.shape) == want[1].shape, what
    assert np.array_equal(walks.cpu().numpy(), want[0].astype(col_dtype)), "walks differ: %s" % what
    assert np.array_equal(eids.cpu().numpy(), want[1]), "edge ids differ: %s" % what


def _assert_follows_edges(walks, eids, row_ptr, col, what):
    """-1 from a walk's end on, in both outputs; every step taken is an edge of the node it was taken from"""
    n_nodes = row_ptr.shape[0] - 1
    assert ((walks >= 0) & (walks < n_nodes) | (walks == -1)).all(), what
    ended = walks[:, 1:] < 0
    assert np.array_equal(ended, eids < 0) and (np.diff(ended.astype(np.int8), axis=1) >= 0).all(), what
    taken, src = eids[~ended], walks[:, :-1][~ended]
    assert np.array_equal(np.asarray(col)[taken].astype(np.int64), walks[:, 1:][~ended]), what
    assert ((taken >= row_ptr[src]) & (taken < row_ptr[src + 1])).all(), what


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("mt,loc,start_dtype,col_dtype", [
    ("continuous", "cuda", "int64", "int64"), ("continuous", "cuda", "int32", "int32"),
    ("chunked", "cuda", "int64", "int64"), ("chunked", "cuda", "int32", "int32"),
    ("chunked", "cuda", "int64", "int32"), ("chunked", "cuda", "int32", "int64"),
    ("continuous", "cpu", "int64", "int64"), ("continuous", "cpu", "int32", "int32"),
    ("chunked", "cpu", "int64", "int64"), ("chunked", "cpu", "int32", "int32")])
def test_walks_on_the_clustered_ladder_equal_the_reference(gpu_env, mt, loc, start_dtype, col_dtype):
    """no weights, float and double weights (the float ones widened), every (p, q) of the host test, col_sorted both ways"""
    import torch
    ref.assert_ladder_measures()
    graph = ref.clustered_ladder()
    g, ts = _structure(gpu_env, mt, loc, NP_OF[col_dtype], graph, [graph[2], graph[2].astype(np.float64)])
    dev_starts = torch.from_numpy(graph[3].astype(NP_OF[start_dtype])).cuda()
    for p, q in ref.PQ:
        for i, wdtype in enumerate(WEIGHTS):
            want = ref.ladder_walks(p, q, wdtype is not None)
            for col_sorted in (False, True):
                got = g.node2vec_walk(dev_starts, ref.LENGTH, p, q, weight_name=None if wdtype is None else "w%d" % (i - 1),
                                      random_seed=ref.SEED, col_sorted=col_sorted, need_edge_ids=True)
                _assert_equal(got, want, NP_OF[col_dtype], "p = %g, q = %g, weights %s, col_sorted %s" % (p, q, wdtype, col_sorted))
    only = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, weight_name="w0", random_seed=ref.SEED, col_sorted=True)
    assert np.array_equal(only.cpu().numpy(), ref.ladder_walks(0.25, 4.0, True)[0].astype(NP_OF[col_dtype])), "walks without edge ids"
    _destroy(ts)


@pytest.mark.parametrize("mt,col_dtype", [("chunked", "int64"), ("continuous", "int32")])
def test_walks_on_the_unsorted_twin_equal_the_reference(gpu_env, mt, col_dtype):
    """the rows in a shuffled order: only the scanning route is defined on them"""
    import torch
    graph = ref.unsorted_twin()
    g, ts = _structure(gpu_env, mt, "cuda", NP_OF[col_dtype], graph, [graph[2]])
    dev_starts = torch.from_numpy(np.array(graph[3])).cuda()
    for p, q in ref.PQ_MEASURED:
        for name in (None, "w0"):
            got = g.node2vec_walk(dev_starts, ref.LENGTH, p, q, weight_name=name, random_seed=ref.SEED, col_sorted=False,
                                  need_edge_ids=True)
            _assert_equal(got, ref.ladder_walks(p, q, name is not None, twin=True), NP_OF[col_dtype],
                          "unsorted twin, p = %g, q = %g, weights %s" % (p, q, name))
    _destroy(ts)


def test_p_q_of_one_is_the_first_order_walk(gpu_env):
    """p = q = 1: with weights, random_walk with the same weight tensor; without, random_walk over a tensor of ones"""
    import torch
    graph = ref.clustered_ladder()
    ones = np.ones(graph[1].shape[0], dtype=np.float32)
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, graph, [graph[2], graph[2].astype(np.float64), ones])
    dev_starts = torch.from_numpy(np.array(graph[3])).cuda()
    for name, plain_name in (("w0", "w0"), ("w1", "w1"), (None, "w2")):
        plain = g.random_walk(dev_starts, ref.LENGTH, weight_name=plain_name, random_seed=ref.SEED, need_edge_ids=True)
        for col_sorted in (False, True):
            got = g.node2vec_walk(dev_starts, ref.LENGTH, 1.0, 1.0, weight_name=name, random_seed=ref.SEED,
                                  col_sorted=col_sorted, need_edge_ids=True)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]), (name, col_sorted)
    assert (plain[1] >= 0).sum() >= 1500
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ damaged graphs, broken promises
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_damaged_col_ind_ends_walks(gpu_env, col_dtype):
    """col_ind entries of -1, n_nodes and 2^31 - 1: they are compared like any id and get some class; the walk that picks one
    ends there, -1 in both outputs, and the call succeeds; every id that IS written indexes row_ptr"""
    import torch
    row_ptr, col, weights, starts = ref.clustered_ladder()
    bad = np.array(col)
    hit = np.arange(3, bad.shape[0], 7)
    bad[hit] = np.array([-1, ref.NODES, (1 << 31) - 1], dtype=np.int64)[np.arange(hit.shape[0]) % 3]
    g, ts = _structure(gpu_env, "chunked", "cuda", NP_OF[col_dtype], (row_ptr, bad), [weights])
    dev_starts = torch.from_numpy(np.array(starts)).cuda()
    for name in (None, "w0"):
        want = ref.node2vec_walks(row_ptr, bad, None if name is None else weights, starts, ref.LENGTH, 0.25, 4.0, ref.SEED)
        assert ((want[0][:, 1:] < 0) & (want[0][:, :-1] >= 0)).sum() >= 100, "too few walks meet a damaged entry"
        got = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, weight_name=name, random_seed=ref.SEED, col_sorted=False,
                              need_edge_ids=True)
        torch.cuda.synchronize()
        _assert_equal(got, want, NP_OF[col_dtype], "damaged, weights %s" % name)
        _assert_follows_edges(got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy(), row_ptr, bad, "damaged")
    _destroy(ts)


def test_a_broken_col_sorted_promise_still_follows_edges(gpu_env):
    """col_sorted=True on the unsorted twin: which class a neighbour gets is not specified, but the call succeeds and every
    step taken is an edge of the node it was taken from"""
    import torch
    graph = ref.unsorted_twin()
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, graph, [graph[2]])
    dev_starts = torch.from_numpy(np.array(graph[3])).cuda()
    for name in (None, "w0"):
        walks, eids = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, weight_name=name, random_seed=ref.SEED, col_sorted=True,
                                      need_edge_ids=True)
        torch.cuda.synchronize()
        walks, eids = walks.cpu().numpy(), eids.cpu().numpy()
        assert (eids >= 0).sum() >= 1500
        _assert_follows_edges(walks, eids, graph[0], graph[1], "broken promise, weights %s" % name)
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ edge cases
def test_empty_batch_batch_independence_and_seeds(gpu_env):
    import torch
    graph = ref.clustered_ladder()
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, graph, [graph[2]])
    dev_starts = torch.from_numpy(np.array(graph[3])).cuda()
    for name in (None, "w0"):
        for col_sorted in (False, True):
            kw = dict(weight_name=name, col_sorted=col_sorted)
            walks, eids = g.node2vec_walk(dev_starts[:0], 4, 0.25, 4.0, random_seed=5, need_edge_ids=True, **kw)
            assert tuple(walks.shape) == (0, 5) and tuple(eids.shape) == (0, 4) and walks.dtype == torch.int64
            whole = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, random_seed=ref.SEED, need_edge_ids=True, **kw)
            first = g.node2vec_walk(dev_starts[:100], ref.LENGTH, 0.25, 4.0, random_seed=ref.SEED, need_edge_ids=True, **kw)
            assert torch.equal(whole[0][:100], first[0]) and torch.equal(whole[1][:100], first[1]), "a walk depends on its batch"
            again = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, random_seed=ref.SEED, need_edge_ids=True, **kw)
            assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1]), "the same seed, other walks"
            a = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, **kw)
            b = g.node2vec_walk(dev_starts, ref.LENGTH, 0.25, 4.0, **kw)
            assert not torch.equal(a, b), "no seed given twice: the same walks"
    _destroy(ts)


@pytest.mark.parametrize("col_sorted", [False, True], ids=["scan", "search"])
def test_many_walks_equal_the_reference(gpu_env, col_sorted):
    """70001 walks of 3 steps on the clustered ladder without its heavy nodes: no multiple of any block size, more than one
    block per CU. Walks 0 .. 255 and the last 255 are compared with the reference, the edge structure of all of them is checked"""
    import torch
    row_ptr, col, weights, _ = ref.clustered_ladder(heavy=False)
    n, length, seed = 70001, 3, 31
    starts = np.random.default_rng(17).integers(-2, ref.NODES + 2, n).astype(np.int32)
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int32, (row_ptr, col), [weights])
    walks, eids = g.node2vec_walk(torch.from_numpy(starts).cuda(), length, 0.25, 4.0, weight_name="w0", random_seed=seed,
                                  col_sorted=col_sorted, need_edge_ids=True)
    walks, eids = walks.cpu().numpy(), eids.cpu().numpy()
    assert walks.dtype == np.int32 and walks.shape == (n, length + 1) and eids.shape == (n, length)
    for first, last in ((0, 256), (n - 255, n)):
        want = ref.node2vec_walks(row_ptr, col, weights, starts[first:last], length, 0.25, 4.0, seed, first_walk=first)
        assert np.array_equal(walks[first:last], want[0]) and np.array_equal(eids[first:last], want[1]), (first, last)
    assert np.array_equal(walks[:, 0], np.where((starts >= 0) & (starts < ref.NODES), starts, -1))
    assert (eids[:, -1] >= 0).sum() >= n // 2
    _assert_follows_edges(walks.astype(np.int64), eids, row_ptr, col, "70001 walks")
    _destroy(ts)


def test_distributed_csr_is_not_implemented(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    graph = ref.clustered_ladder()
    dev_starts = torch.from_numpy(np.array(graph[3])).cuda()
    g, ts = _structure(gpu_env, "distributed", "cuda", np.int64, graph)
    with pytest.raises(binding.WholeMemoryError) as e:
        g.node2vec_walk(dev_starts, 3, 0.5, 2.0, random_seed=1)
    assert e.value.code == 2 and isinstance(e.value, NotImplementedError)      # WHOLEMEMORY_NOT_IMPLEMENTED
    _destroy(ts)
    ts = [_wm_array(gpu_env, "chunked", graph[0]), _wm_array(gpu_env, "distributed", graph[1])]      # col_ind alone
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    with pytest.raises(binding.WholeMemoryError) as e:
        g.node2vec_walk(dev_starts, 3, 0.5, 2.0, random_seed=1, col_sorted=True)
    assert e.value.code == 2
    _destroy(ts)
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, graph)
    ts.append(_wm_array(gpu_env, "distributed", graph[2]))
    g.set_edge_attribute("w", ts[2])
    with pytest.raises(binding.WholeMemoryError) as e:
        g.node2vec_walk(dev_starts, 3, 0.5, 2.0, weight_name="w", random_seed=1)
    assert e.value.code == 2
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_second_step_on_the_kite_follows_the_biases(gpu_env, weighted):
    """24 000 walks of 2 steps from node 1 of the kite, (p, q) = (0.5, 2): among the walks through node 0 the second step fits
    {1: 1 / p; 2, 3: 1; 4, 5, 6: 1 / q} (times the weights 1 .. 6 in the weighted form): chi-square over 5 degrees of freedom
    below 40, the bar of tests/test_sampler_edges_gpu.py — and equal to the value the host program gave
    (tests/test_n2v_streams.py), because these are the same walks."""
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    row_ptr, col, weights = ref.kite()
    hold = [torch.from_numpy(a).cuda() for a in (row_ptr, col, weights)]
    wr, wc, ww = [wrap_torch_tensor(t) for t in hold]
    starts = torch.ones(ref.KITE_WALKS, dtype=torch.int64, device="cuda")
    values = []
    for col_sorted in (False, True):
        walks = wops.node2vec_walk(wr.handle, wc.handle, starts, ref.KITE_LENGTH, ref.KITE_P, ref.KITE_Q, ref.KITE_SEED,
                                   wm_csr_weight_ptr_tensor=ww.handle if weighted else None, col_sorted=col_sorted)
        values.append(ref.kite_statistic(walks.cpu().numpy(), weighted))
    print("kite, %s: chi-square %.4f (scan), %.4f (search) over 5 dof" % ("weighted" if weighted else "unweighted", *values))
    for chi2 in values:
        assert chi2 < 40.0, "chi-square %.1f over 5 dof" % chi2
        assert abs(chi2 - ref.KITE_CHI2[weighted]) < 1e-6, (chi2, ref.KITE_CHI2[weighted])
