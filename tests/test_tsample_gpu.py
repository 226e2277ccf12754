"""Temporal neighbour sampling on the MI355X (csrc/kernels/tsample.hip through wholegraph_ops.temporal_sample_without_replacement
/ GraphStructure.temporal_sample_one_hop) against the definition restated in Python (tests/_tsample_ref.py), bit for bit.

The temporal ladder: the ladder of tests/_walk_ref.py (2000 nodes; nodes 7 .. 15 with 5000, 1024, 1025, 63, 64, 0, 1, 65 and 2
neighbours) with its 512 starts as centres, edge times in [0, 1000) with a row of one value, an ascending row, a row in every
centre's future and a row of INT64_MIN / INT64_MAX, centre times in [0, 1000) and at INT64_MIN, INT64_MAX and 0. The reference
outputs are computed once and shared. Also: the first 100 centres alone, 70 001 centres (more than one trip of the capped
grid), graph and time tensors that are sub-tensor views at odd storage offsets, plain device tensors, degenerate and damaged
inputs, the Python-side route for DISTRIBUTED tensors, and the octet, whose statistics are those of the reference."""
import numpy as np
import pytest

import _tsample_ref as ref

pytestmark = pytest.mark.gpu

NP_OF = {"int32": np.int32, "int64": np.int64}
NAMES = ("offsets", "ids", "center local ids", "edge ids")


def _wm_array(comm, mt, arr, loc="cuda"):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr), loc)        # (a writable copy: the shared arrays are read-only)


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm, mt, loc, col_dtype, row_ptr, col, edge_time):
    import wholegraph_amd.torch as wgth
    ts = [_wm_array(comm, mt, row_ptr, loc), _wm_array(comm, mt, np.asarray(col).astype(col_dtype), loc),
          _wm_array(comm, mt, edge_time, loc)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("t", ts[2])
    return g, ts


def _assert_equal(got, want, lid, eid, what):
    """got: the op's tuple of device tensors; want: the reference's (offsets, ids, center local ids, edge ids, ...)"""
    import torch
    expect = [(NAMES[0], want[0]), (NAMES[1], want[1])] + ([(NAMES[2], want[2])] if lid else []) + ([(NAMES[3], want[3])] if eid else [])
    assert len(got) == len(expect), what
    for a, (name, b) in zip(got, expect):
        assert a.is_cuda and tuple(a.shape) == b.shape, "%s: %s" % (name, what)
        if name != NAMES[1]:
            assert a.dtype == torch.from_numpy(np.empty(0, dtype=b.dtype)).dtype, "%s: %s" % (name, what)
        assert np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)), "%s differ: %s" % (name, what)


def _dev(a, dtype=np.int64):
    import torch
    return torch.from_numpy(np.array(a).astype(dtype)).cuda()


# ------------------------------------------------------------------------------------------------ parity on the ladder
def test_the_ladder_keeps_its_cases():
    """lower bounds on the REFERENCE, so that a later change of the ladder cannot empty a case"""
    print("the temporal ladder at M = %d: %s" % (ref.LADDER_M, ref.assert_ladder_measures()))


@pytest.mark.parametrize("mt,loc", [("continuous", "cuda"), ("chunked", "cuda"), ("continuous", "cpu"), ("chunked", "cpu")])
@pytest.mark.parametrize("center_dtype,col_dtype", [("int64", "int64"), ("int32", "int32"), ("int64", "int32"), ("int32", "int64")])
def test_the_ladder_sample_equals_the_reference(gpu_env, mt, loc, center_dtype, col_dtype):
    import torch
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    want = ref.ladder_sample()
    g, ts = _structure(gpu_env, mt, loc, NP_OF[col_dtype], row_ptr, col, etime)
    centres, times = _dev(starts, NP_OF[center_dtype]), _dev(ctimes)
    what = "%s / %s, centres %s, col %s" % (mt, loc, center_dtype, col_dtype)
    for lid, eid in ((True, True), (False, False), (True, False), (False, True)):
        got = g.temporal_sample_one_hop("t", centres, times, ref.LADDER_M, random_seed=ref.LADDER_SEED,
                                        need_center_local_output=lid, need_edge_output=eid)
        assert got[1].dtype == (torch.int32 if col_dtype == "int32" else torch.int64)
        _assert_equal(got, want, lid, eid, "%s, outputs %s %s" % (what, lid, eid))
    # inclusive=False holds the centre with exactly M eligible neighbours (batch position 9)
    earlier = ref.ladder_sample(inclusive=False)
    assert earlier[4][9] == ref.LADDER_M
    got = g.temporal_sample_one_hop("t", centres, times, ref.LADDER_M, inclusive=False, random_seed=ref.LADDER_SEED,
                                    need_center_local_output=True, need_edge_output=True)
    _assert_equal(got, earlier, True, True, what + ", inclusive=False")
    _destroy(ts)


@pytest.mark.parametrize("strategy", ["uniform", "last"])
@pytest.mark.parametrize("m", [1, 5, 32, 33, 64, -1])
def test_every_rule_on_one_layout(gpu_env, m, strategy):
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, row_ptr, col, etime)
    centres, times = _dev(starts), _dev(ctimes)
    for inclusive in (True, False):
        for window in (None, 0, 50):
            want = ref.ladder_sample(m, strategy, inclusive, window)
            what = "M = %d, %s, inclusive %s, window %s" % (m, strategy, inclusive, window)
            for flag in (True, False):
                got = g.temporal_sample_one_hop("t", centres, times, m, strategy=strategy, inclusive=inclusive, time_window=window,
                                                random_seed=ref.LADDER_SEED, need_center_local_output=flag, need_edge_output=flag)
                _assert_equal(got, want, flag, flag, what)
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ geometry
def test_the_first_100_centres_alone_give_the_same_rows(gpu_env):
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int64, row_ptr, col, etime)
    for strategy in ("uniform", "last"):
        want = ref.ladder_sample(ref.LADDER_M, strategy)
        cut = int(want[0][100])
        got = g.temporal_sample_one_hop("t", _dev(starts[:100]), _dev(ctimes[:100]), ref.LADDER_M, strategy=strategy,
                                        random_seed=ref.LADDER_SEED, need_center_local_output=True, need_edge_output=True)
        _assert_equal(got, (want[0][:101], want[1][:cut], want[2][:cut], want[3][:cut]), True, True, "the first 100, " + strategy)
    _destroy(ts)


@pytest.mark.parametrize("center_dtype,col_dtype", [("int32", "int32"), ("int64", "int64")])
def test_70001_centres_take_more_than_one_grid_trip(gpu_env, center_dtype, col_dtype):
    """the ladder batch tiled to 70 001 centres: no multiple of a block, more blocks than the capped grid of either kernel has
    (2048 blocks of 16 and of 8 centres), so later trips of both grid-stride loops run; a tiled position has its own streams,
    so the reference is computed for all 70 001; two calls agree"""
    import torch
    row_ptr, col, etime, _, _ = ref.temporal_ladder()
    centres, times, want = ref.tiled_ladder()
    assert centres.shape[0] == 70001 > 2048 * 16 and want[0][-1] >= 200000
    g, ts = _structure(gpu_env, "chunked", "cuda", NP_OF[col_dtype], row_ptr, col, etime)
    dev, dev_t = _dev(centres, NP_OF[center_dtype]), _dev(times)
    got = g.temporal_sample_one_hop("t", dev, dev_t, ref.LADDER_M, random_seed=ref.LADDER_SEED, need_center_local_output=True,
                                    need_edge_output=True)
    _assert_equal(got, want, True, True, "70 001 centres")
    again = g.temporal_sample_one_hop("t", dev, dev_t, ref.LADDER_M, random_seed=ref.LADDER_SEED, need_center_local_output=True,
                                      need_edge_output=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two calls differ"
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("mt,col_dtype", [("continuous", np.int32), ("continuous", np.int64), ("chunked", np.int32),
                                          ("chunked", np.int64)])
def test_graph_and_time_tensors_at_odd_storage_offsets(gpu_env, mt, col_dtype):
    """row_ptr a view from element 3, col_ind from element 5 and the edge times from element 7 of poisoned arrays (a large
    negative number, an id that is no node, a time that every centre passes): an offset dropped or swapped reads the poison"""
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    roots, views = [], []
    for arr, lead, poison in ((row_ptr, 3, -(1 << 40)), (col.astype(col_dtype), 5, 2000 + 12345), (etime, 7, ref.INT64_MIN)):
        padded = np.full(lead + arr.shape[0] + 6, poison, dtype=arr.dtype)
        padded[lead:lead + arr.shape[0]] = arr
        root = _wm_array(gpu_env, mt, padded)
        view = root.get_sub_tensor([lead], [lead + arr.shape[0]])
        assert view.storage_offset() == lead and tuple(view.shape) == (arr.shape[0],)
        roots.append(root)
        views.append(view)
    for strategy in ("uniform", "last"):
        got = wops.temporal_sample_without_replacement(views[0].wmb_tensor, views[1].wmb_tensor, views[2].wmb_tensor, _dev(starts),
                                                       _dev(ctimes), ref.LADDER_M, ref.LADDER_SEED, True, True, strategy=strategy)
        _assert_equal(got, ref.ladder_sample(ref.LADDER_M, strategy), True, True, "offset views, %s, %s" % (mt, strategy))
    for t in views + roots:
        wgth.destroy_wholememory_tensor(t)


def test_plain_device_tensors(gpu_env):
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    hold = [_dev(row_ptr), _dev(col, np.int32), _dev(etime)]
    wr, wc, wt = [wrap_torch_tensor(t) for t in hold]
    got = wops.temporal_sample_without_replacement(wr.handle, wc.handle, wt.handle, _dev(starts, np.int32), _dev(ctimes), ref.LADDER_M,
                                                   ref.LADDER_SEED, True, True)
    _assert_equal(got, ref.ladder_sample(), True, True, "plain device tensors")


# ------------------------------------------------------------------------------------------------ degenerate and damaged inputs
def test_no_centres_and_a_graph_without_edges(gpu_env):
    import torch
    row_ptr, col, etime, _, _ = ref.temporal_ladder()
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int32, row_ptr, col, etime)
    for dtype in (torch.int32, torch.int64):
        got = g.temporal_sample_one_hop("t", torch.empty(0, dtype=dtype, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                                        5, need_center_local_output=True, need_edge_output=True)
        assert got[0].dtype == torch.int32 and got[0].tolist() == [0]
        assert [tuple(t.shape) for t in got[1:]] == [(0,)] * 3
        assert [t.dtype for t in got[1:]] == [torch.int32, torch.int32, torch.int64]
    refused = torch.tensor([-1, 2000, 2005, -7, (1 << 31) - 1, 1 << 40], dtype=torch.int64, device="cuda")
    got = g.temporal_sample_one_hop("t", refused, torch.full((6,), 999, dtype=torch.int64, device="cuda"), -1, need_edge_output=True)
    assert got[0].tolist() == [0] * 7 and got[1].numel() == 0 and got[2].numel() == 0
    _destroy(ts)
    # a graph without edges, as plain device tensors
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    hold = [torch.zeros(6, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
            torch.empty(0, dtype=torch.int64, device="cuda")]
    wr, wc, wt = [wrap_torch_tensor(t) for t in hold]
    got = wops.temporal_sample_without_replacement(wr.handle, wc.handle, wt.handle, _dev([0, 4, 5, 2]), _dev([1, 2, 3, 4]), 3, 9, True)
    assert got[0].tolist() == [0] * 5 and got[1].numel() == 0 and got[2].numel() == 0


def test_damaged_row_ptr_gives_empty_rows(gpu_env):
    """five nodes; the pair of node 1 has e < s and the pairs of nodes 3 and 4 leave the edge array: those rows are empty, the
    others right"""
    row_ptr = np.array([0, 3, 2, 5, 9, 7], dtype=np.int64)      # rows: [0, 3), (3, 2) damaged, [2, 5), (5, 9) damaged, (9, 7) damaged
    col = np.array([1, 2, 0, 4, 3, 0, 2], dtype=np.int64)
    etime = np.array([5, 1, 9, 2, 7, 3, 3], dtype=np.int64)
    centres, times = np.array([4, 3, 2, 1, 0, 2], dtype=np.int64), np.array([9, 9, 8, 9, 5, 2], dtype=np.int64)
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int64, row_ptr, col, etime)
    for m, rows in ((-1, [0, 0, 2, 0, 2, 1]), (2, [0, 0, 2, 0, 2, 1]), (1, [0, 0, 1, 0, 1, 1])):
        want = ref.temporal_sample(row_ptr, col, etime, centres, times, m, "last", True, None, 1)
        assert np.diff(want[0]).tolist() == rows
        got = g.temporal_sample_one_hop("t", _dev(centres), _dev(times), m, strategy="last", random_seed=1,
                                        need_center_local_output=True, need_edge_output=True)
        _assert_equal(got, want, True, True, "damaged row_ptr, M = %d" % m)
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ DISTRIBUTED, on one rank
@pytest.mark.parametrize("which", ["all", "times"])
def test_distributed_tensors_give_the_reference_samples(gpu_env, which):
    """the C entry point answers NOT_IMPLEMENTED; the Python op composes the route, and i and j are preserved by it"""
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd import binding
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    graph_mt = "distributed" if which == "all" else "chunked"
    ts = [_wm_array(gpu_env, graph_mt, row_ptr), _wm_array(gpu_env, graph_mt, col), _wm_array(gpu_env, "distributed", etime)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("t", ts[2])
    centres, times = _dev(starts), _dev(ctimes)
    with pytest.raises(binding.WholeMemoryError) as e:
        wops._temporal_sample_mapped(ts[0].wmb_tensor, ts[1].wmb_tensor, ts[2].wmb_tensor, centres, times, 5, 1, False, False, (0, True, -1))
    assert e.value.code == 2      # WHOLEMEMORY_NOT_IMPLEMENTED
    for strategy, m, window in (("uniform", ref.LADDER_M, None), ("last", 5, 50), ("uniform", -1, None)):
        want = ref.ladder_sample(m, strategy, True, window)
        for flag in (True, False):
            got = g.temporal_sample_one_hop("t", centres, times, m, strategy=strategy, time_window=window, random_seed=ref.LADDER_SEED,
                                            need_center_local_output=flag, need_edge_output=flag)
            _assert_equal(got, want, flag, flag, "DISTRIBUTED %s, %s, M = %d" % (which, strategy, m))
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ uniformity
def test_the_octet_is_uniform(gpu_env):
    """6000 centres, all the node with 8 neighbours at times 1 .. 8, at time 6, inclusive, M = 2, seed 31415: the output equals
    the reference, whose statistics were computed on the CPU from the restated contract before any kernel existed (chi-square
    1.586 over 5 degrees of freedom for the six eligible neighbours, 7.92 over 14 for the 15 pairs; the 1 % points are 15.09
    and 29.14); positions 6 and 7 never appear"""
    row_ptr, col, etime = ref.octet()
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int64, row_ptr, col, etime)
    got = g.temporal_sample_one_hop("t", _dev(np.zeros(ref.OCTET_CENTRES)), _dev(np.full(ref.OCTET_CENTRES, ref.OCTET_TIME)),
                                    ref.OCTET_M, random_seed=ref.OCTET_SEED, need_center_local_output=True, need_edge_output=True)
    _assert_equal(got, ref.octet_sample(), True, True, "the octet")
    single, pairs = ref.octet_statistics(got[0].cpu().numpy(), got[3].cpu().numpy())
    print("the octet on the device: chi-square %.4f over 5 dof, %.4f over 14 dof" % (single, pairs))
    assert abs(single - 1.586) < 1e-9 and abs(pairs - 7.92) < 1e-9 and single < 15.09 and pairs < 29.14
    assert not np.isin(got[3].cpu().numpy(), (6, 7)).any()
    _destroy(ts)
