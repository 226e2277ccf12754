"""Negative sampling on the MI355X (csrc/kernels/neg_sample.hip through wholegraph_ops.negative_sample /
GraphStructure.negative_sample) against the definition restated in Python (tests/_neg_ref.py), bit for bit.

The ladder of tests/_walk_ref.py (2000 nodes; nodes 7 .. 15 with 5000, 1024, 1025, 63, 64, 0, 1, 65 and 2 neighbours, a fifth
of the entries redirected to those nine) puts rows around the group size and far above it, an empty row and three refused ids
among 512 sources; its rows are in no order, so only the scanning route is defined on it, and its row-sorted copy takes both
routes, which must agree. The reference outputs are computed once and shared. Also: a damaged graph, the complete graph (where
every candidate is excluded), the statistics of the dozen, the independence of a source from its batch, seeds, an empty batch,
a batch that is no multiple of a block, plain device tensors and the DISTRIBUTED answer."""
import numpy as np
import pytest

import _neg_ref as ref

pytestmark = pytest.mark.gpu

NP_OF = {"int32": np.int32, "int64": np.int64}
MODE_NAMES = {0: "uniform", 1: "degree"}


def _wm_array(comm, mt, arr, loc="cuda"):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr), loc)        # (a writable copy: the shared arrays are read-only)


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm, mt, loc, col_dtype, graph):
    import wholegraph_amd.torch as wgth
    ts = [_wm_array(comm, mt, graph[0], loc), _wm_array(comm, mt, np.asarray(graph[1]).astype(col_dtype), loc)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    return g, ts


def _draw(g, dev_src, k, mode, exclude, tries, seed, col_sorted):
    return g.negative_sample(dev_src, k, mode=MODE_NAMES[mode], exclude_edges=bool(exclude & 1), exclude_self=bool(exclude & 2),
                             max_tries=tries, random_seed=seed, col_sorted=col_sorted)


def _assert_equal(got, want, col_dtype, what):
    import torch
    assert got.dtype == torch.from_numpy(np.empty(0, dtype=col_dtype)).dtype and tuple(got.shape) == want.shape, what
    assert np.array_equal(got.cpu().numpy(), want.astype(col_dtype)), "negatives differ: %s" % what


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("mt,loc", [("continuous", "cuda"), ("chunked", "cuda"), ("continuous", "cpu"), ("chunked", "cpu")])
@pytest.mark.parametrize("src_dtype,col_dtype,modes", [("int64", "int64", (0, 1)), ("int32", "int32", (1,)),
                                                       ("int64", "int32", (0,)), ("int32", "int64", (1,))])
def test_negatives_on_the_ladder_equal_the_reference(gpu_env, mt, loc, src_dtype, col_dtype, modes):
    """K in {1, 5, 33}, exclude 0 .. 3, T in {1, 8}: the ladder by the scanning route, its sorted copy by both routes"""
    import torch
    for in_order in (False, True):
        graph = ref.ladder(in_order)
        g, ts = _structure(gpu_env, mt, loc, NP_OF[col_dtype], graph)
        dev_src = torch.from_numpy(graph[2].astype(NP_OF[src_dtype])).cuda()
        for mode in modes:
            for k in ref.KS:
                for exclude in range(4):
                    for tries in ref.TRIES:
                        want = ref.ladder_negatives(in_order, k, mode, exclude, tries)
                        for col_sorted in ((False, True) if in_order else (False,)):
                            got = _draw(g, dev_src, k, mode, exclude, tries, ref.SEED, col_sorted)
                            _assert_equal(got, want, NP_OF[col_dtype], "sorted copy %s, mode %d, K = %d, exclude %d, T = %d, "
                                          "col_sorted %s" % (in_order, mode, k, exclude, tries, col_sorted))
        _destroy(ts)


# ------------------------------------------------------------------------------------------------ damaged and complete graphs
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_damaged_col_ind_is_refused_not_followed(gpu_env, col_dtype):
    """col_ind entries of -1, n_nodes and 2^31 - 1 (the graph of tests/test_neg_streams.py): drawn in mode 1 and compared in
    the rows like any id, range-checked before anything else; the outputs equal the reference and hold none of them"""
    import torch
    from test_neg_streams import DAMAGED, small_graphs
    in_order, shuffled = small_graphs()
    refused = {}
    for name, graph, routes in (("sorted", in_order, (False, True)), ("shuffled", shuffled, (False,))):
        g, ts = _structure(gpu_env, "chunked", "cuda", NP_OF[col_dtype], graph)
        dev_src = torch.from_numpy(np.array(graph[2])).cuda()
        for mode in (0, 1):
            for exclude in (0, 3):
                want = ref.negative_samples(graph[0], graph[1], graph[2], 33, mode, exclude, 8, 77, out_of_range=refused)
                for col_sorted in routes:
                    got = _draw(g, dev_src, 33, mode, exclude, 8, 77, col_sorted)
                    torch.cuda.synchronize()
                    _assert_equal(got, want, NP_OF[col_dtype], "%s, mode %d, exclude %d, col_sorted %s" % (name, mode, exclude, col_sorted))
                    out = got.cpu().numpy().astype(np.int64)
                    assert ((out == -1) | ((out >= 0) & (out < 60))).all()
        _destroy(ts)
    assert refused and set(refused) <= set(DAMAGED), "no damaged entry was drawn: %s" % refused


@pytest.mark.parametrize("mode", [0, 1], ids=["uniform", "degree"])
def test_complete_graph_leaves_nothing_to_draw(gpu_env, mode):
    """9 nodes, every node the neighbour of every other: with exclude = 3 every output is -1; with exclude = 1 only the source
    itself comes back (64 tries: a sample misses the source with probability (8 / 9)^64 < 0.1 %)"""
    import torch
    nodes = 9
    row_ptr = np.arange(nodes + 1, dtype=np.int64) * (nodes - 1)
    col = np.concatenate([np.delete(np.arange(nodes), v) for v in range(nodes)]).astype(np.int64)
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int64, (row_ptr, col))
    src = np.arange(200, dtype=np.int64) % nodes
    dev_src = torch.from_numpy(src).cuda()
    for col_sorted in (False, True):
        out = _draw(g, dev_src, 20, mode, 3, 64, 5, col_sorted).cpu().numpy()
        assert out.shape == (200, 20) and (out == -1).all()
        out = _draw(g, dev_src, 20, mode, 1, 64, 5, col_sorted).cpu().numpy()
        assert ((out == src[:, None]) | (out == -1)).all() and (out == src[:, None]).mean() >= 0.99
        _assert_equal(torch.from_numpy(out), ref.negative_samples(row_ptr, col, src, 20, mode, 1, 64, 5), np.int64, "complete")
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ distribution
@pytest.mark.parametrize("mode,tries", sorted(ref.DOZEN_VALUES))
def test_the_dozen_reproduces_the_recorded_statistics(gpu_env, mode, tries):
    """3000 x 8 negatives of node 0 of the dozen, exclude = 3: outputs in 6 .. 11, chi-square over 5 degrees of freedom below
    40 — and equal to the value the host program gave (tests/test_neg_streams.py), as is the number of
    outputs that are -1, because these are the same samples"""
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    row_ptr, col = ref.dozen()
    hold = [torch.from_numpy(a).cuda() for a in (row_ptr, col)]
    wr, wc = [wrap_torch_tensor(t) for t in hold]
    src = torch.zeros(ref.DOZEN_SOURCES, dtype=torch.int64, device="cuda")
    missing, recorded = ref.DOZEN_VALUES[(mode, tries)]
    for col_sorted in (False, True):
        out = wops.negative_sample(wr.handle, wc.handle, src, ref.DOZEN_K, ref.DOZEN_SEED, mode=MODE_NAMES[mode], max_tries=tries,
                                   col_sorted=col_sorted).cpu().numpy()
        share, chi2 = ref.dozen_statistic(out, mode)
        print("the dozen, mode %d, T = %d, col_sorted %s: %d are -1, chi-square %.4f" % (mode, tries, col_sorted,
                                                                                         round(share * out.size), chi2))
        assert chi2 < 40.0
        assert share <= 0.001 if tries == 16 else 0.05 <= share <= 0.075
        assert round(share * out.size) == missing and abs(chi2 - recorded) < 1e-6, (share * out.size, chi2, missing, recorded)


# ------------------------------------------------------------------------------------------------ batches and shapes
def test_empty_batch_batch_independence_and_seeds(gpu_env):
    import torch
    graph = ref.ladder(True)
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, graph)
    dev_src = torch.from_numpy(np.array(graph[2])).cuda()
    for mode in ("uniform", "degree"):
        for col_sorted in (False, True):
            kw = dict(mode=mode, col_sorted=col_sorted)
            none = g.negative_sample(dev_src[:0], 5, random_seed=5, **kw)
            assert tuple(none.shape) == (0, 5) and none.dtype == torch.int64
            whole = g.negative_sample(dev_src, 5, random_seed=ref.SEED, **kw)
            first = g.negative_sample(dev_src[:100], 5, random_seed=ref.SEED, **kw)
            assert torch.equal(whole[:100], first), "a source depends on its batch"
            assert torch.equal(whole, g.negative_sample(dev_src, 5, random_seed=ref.SEED, **kw)), "the same seed, other samples"
            other = g.negative_sample(dev_src, 5, random_seed=ref.SEED + 1, **kw)
            assert (other != whole).float().mean() > 0.9, "another seed, the same samples"
            a, b = g.negative_sample(dev_src, 5, **kw), g.negative_sample(dev_src, 5, **kw)
            assert not torch.equal(a, b), "no seed given twice: the same samples"
    # the defaults: uniform, neighbours and the source excluded, 8 tries, the scanning route
    _assert_equal(g.negative_sample(dev_src, 5, random_seed=ref.SEED), ref.ladder_negatives(True, 5, 0, 3, 8), np.int64, "defaults")
    _destroy(ts)


@pytest.mark.parametrize("col_sorted", [False, True], ids=["scan", "search"])
def test_many_sources_equal_the_reference(gpu_env, col_sorted):
    """70001 sources with K = 3 on the sorted ladder: no multiple of any block size, more than one block per CU. 2000 rows —
    the first and the last 256 among them — are compared with the reference; every output is checked against its source"""
    import torch
    row_ptr, col, _ = ref.ladder(True)
    n, k, seed = 70001, 3, 31
    src = np.random.default_rng(17).integers(-2, 2002, n).astype(np.int32)
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int32, (row_ptr, col))
    out = g.negative_sample(torch.from_numpy(src).cuda(), k, mode="degree", random_seed=seed, col_sorted=col_sorted).cpu().numpy()
    assert out.dtype == np.int32 and out.shape == (n, k)
    rows = np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), np.random.default_rng(3).integers(0, n, 1600)]))[:2000]
    want = ref.negative_samples(row_ptr, col, src[rows], k, 1, 3, 8, seed, numbers=rows)
    assert np.array_equal(out[rows], want)
    inside = (src >= 0) & (src < 2000)
    assert (out[~inside] == -1).all() and (~inside).sum() >= 50 and (out[inside] >= 0).mean() > 0.95
    assert not (out == src[:, None])[inside].any() and out.max() < 2000 and out.min() >= -1
    _destroy(ts)


def test_plain_device_tensors_and_a_flat_output(gpu_env):
    """plain device arrays wrapped as tensors; the output given as 1-D with n * K entries through the C entry point"""
    import ctypes as C
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import get_stream, wrap_torch_tensor
    row_ptr, col, src = ref.ladder(True)
    hold = [torch.from_numpy(np.array(a)).cuda() for a in (row_ptr, col.astype(np.int32))]
    wr, wc = [wrap_torch_tensor(t) for t in hold]
    dev_src = torch.from_numpy(np.array(src)).cuda()
    got = wops.negative_sample(wr.handle, wc.handle, dev_src, 5, ref.SEED, mode="degree", col_sorted=True)
    _assert_equal(got, ref.ladder_negatives(True, 5, 1, 3, 8), np.int32, "plain device tensors")
    flat = torch.full((src.shape[0] * 5,), -7, dtype=torch.int32, device="cuda")
    ws, wf = wrap_torch_tensor(dev_src), wrap_torch_tensor(flat)
    wmb.check(wmb.lib().wholememory_ext_csr_negative_sample(wr.handle, wc.handle, ws.handle, 5, 1, 3, 8, 1, C.c_ulonglong(ref.SEED),
                                                            wf.handle, C.c_void_p(get_stream())))
    assert torch.equal(flat.reshape(-1, 5), got)


def test_distributed_csr_is_not_implemented(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    graph = ref.ladder(True)
    dev_src = torch.from_numpy(np.array(graph[2])).cuda()
    g, ts = _structure(gpu_env, "distributed", "cuda", np.int64, graph)
    with pytest.raises(binding.WholeMemoryError) as e:
        g.negative_sample(dev_src, 5, random_seed=1)
    assert e.value.code == 2 and isinstance(e.value, NotImplementedError)      # WHOLEMEMORY_NOT_IMPLEMENTED
    _destroy(ts)
    ts = [_wm_array(gpu_env, "chunked", graph[0]), _wm_array(gpu_env, "distributed", graph[1])]      # col_ind alone
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    with pytest.raises(binding.WholeMemoryError) as e:
        g.negative_sample(dev_src, 5, random_seed=1, col_sorted=True, exclude_edges=False)
    assert e.value.code == 2
    _destroy(ts)
