"""The node-induced subgraph on the MI355X (csrc/kernels/isub.hip through wholegraph_ops.induced_subgraph /
GraphStructure.induced_subgraph) against the definition restated in Python (tests/_isub_ref.py), bit for bit.

The ladder of tests/_walk_ref.py (2000 nodes; nodes 7 .. 15 with 5000, 1024, 1025, 63, 64, 0, 1, 65 and 2 neighbours, a fifth
of the entries redirected to those nine) with its 512 starts as the node list: duplicate positions, three ids that are no
nodes, rows far above, at and around the group size, rows kept in part and rows that end up empty. The reference outputs are
computed once and shared. Also: the whole graph under a permutation, degenerate lists, damaged graphs, 70 001 rows, graph
tensors that are sub-tensor views at odd storage offsets, a subgraph of 2.4e9 entries (refused after the count), plain device
tensors and the DISTRIBUTED answer."""
import numpy as np
import pytest

import _isub_ref as ref
from _walk_ref import LADDER_NODES, ladder

pytestmark = pytest.mark.gpu

NP_OF = {"int32": np.int32, "int64": np.int64}


def _wm_array(comm, mt, arr, loc="cuda"):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr), loc)        # (a writable copy: the shared arrays are read-only)


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm, mt, loc, col_dtype, row_ptr, col):
    import wholegraph_amd.torch as wgth
    ts = [_wm_array(comm, mt, row_ptr, loc), _wm_array(comm, mt, np.asarray(col).astype(col_dtype), loc)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    return g, ts


def _assert_equal(got, want, what):
    """got: the op's tuple of device tensors; want: the reference's (offsets, col, edge ids), cut to as many"""
    import torch
    assert len(got) in (2, 3), what
    for name, a, b in zip(("offsets", "col", "edge ids"), got, want):
        assert a.is_cuda and a.dtype == torch.from_numpy(np.empty(0, dtype=b.dtype)).dtype and tuple(a.shape) == b.shape, "%s: %s" % (name, what)
        assert np.array_equal(a.cpu().numpy(), b), "%s differ: %s" % (name, what)


# ------------------------------------------------------------------------------------------------ parity on the ladder
def test_the_ladder_keeps_its_cases():
    """lower bounds on the REFERENCE, so that a later change of the ladder cannot empty a case"""
    m = ref.ladder_measures()
    print("the ladder's subgraph: %s" % m)
    assert m["m"] >= 3000 and m["row_of_7"] >= 1000 and m["empty_rows"] >= 50 and m["duplicates"] >= 30 and m["refused"] == 3, m
    assert m["partial_rows"] >= 100 and all(1 <= v for v in m["rows"].values()), m


@pytest.mark.parametrize("mt,loc", [("continuous", "cuda"), ("chunked", "cuda"), ("continuous", "cpu"), ("chunked", "cpu")])
@pytest.mark.parametrize("node_dtype,col_dtype", [("int64", "int64"), ("int32", "int32"), ("int64", "int32"), ("int32", "int64")])
def test_the_ladder_subgraph_equals_the_reference(gpu_env, mt, loc, node_dtype, col_dtype):
    import torch
    row_ptr, col, _, starts = ladder()
    want = ref.ladder_subgraph()
    g, ts = _structure(gpu_env, mt, loc, NP_OF[col_dtype], row_ptr, col)
    nodes = torch.from_numpy(starts.astype(NP_OF[node_dtype])).cuda()
    what = "%s / %s, nodes %s, col %s" % (mt, loc, node_dtype, col_dtype)
    without = g.induced_subgraph(nodes)
    assert len(without) == 2
    _assert_equal(without, want, what)
    with_ids = g.induced_subgraph(nodes, need_edge_output=True)
    assert len(with_ids) == 3
    _assert_equal(with_ids, want, what + ", with edge ids")
    _destroy(ts)


def test_edge_attributes_of_the_kept_edges(gpu_env):
    """the attribute dict of GraphStructure.induced_subgraph equals attr[edge ids]"""
    import torch
    row_ptr, col, weights, starts = ladder()
    want = ref.ladder_subgraph()
    g, ts = _structure(gpu_env, "chunked", "cuda", np.int64, row_ptr, col)
    tag = np.arange(col.shape[0], dtype=np.int64) * 3 + 1
    ts += [_wm_array(gpu_env, "chunked", weights), _wm_array(gpu_env, "continuous", tag)]
    g.set_edge_attribute("w", ts[2])
    g.set_edge_attribute("tag", ts[3])
    nodes = torch.from_numpy(np.array(starts)).cuda()
    offsets, out_col, attrs = g.induced_subgraph(nodes, edge_attr_names=["w", "__edge_id__", "tag"])
    _assert_equal((offsets, out_col), want, "with attributes")
    assert sorted(attrs) == ["__edge_id__", "tag", "w"]
    assert np.array_equal(attrs["__edge_id__"].cpu().numpy(), want[2])
    assert np.array_equal(attrs["w"].cpu().numpy(), weights[want[2]]) and np.array_equal(attrs["tag"].cpu().numpy(), tag[want[2]])
    four = g.induced_subgraph(nodes, need_edge_output=True, edge_attr_names=["tag"])
    assert len(four) == 4 and list(four[3]) == ["tag"] and torch.equal(four[3]["tag"], attrs["tag"])
    _assert_equal(four[:3], want, "with edge ids and attributes")
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ the whole graph
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_a_permutation_of_all_nodes_keeps_every_edge(gpu_env, col_dtype):
    import torch
    row_ptr, col, _, _ = ladder()
    perm = np.random.default_rng(11).permutation(LADDER_NODES).astype(np.int64)
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(LADDER_NODES)
    g, ts = _structure(gpu_env, "chunked", "cuda", NP_OF[col_dtype], row_ptr, col)
    offsets, out_col, eid = (t.cpu().numpy() for t in g.induced_subgraph(torch.from_numpy(perm).cuda(), need_edge_output=True))
    assert offsets[-1] == col.shape[0] == out_col.shape[0] == eid.shape[0]
    assert np.array_equal(np.diff(offsets.astype(np.int64)), (row_ptr[1:] - row_ptr[:-1])[perm])
    want_eid = np.concatenate([np.arange(row_ptr[u], row_ptr[u + 1]) for u in perm])
    assert np.array_equal(eid, want_eid), "the edge ids of row i are not range(row_ptr[u], row_ptr[u + 1])"
    assert np.array_equal(out_col, inverse[col[want_eid]].astype(np.int32)), "col is not the inverse permutation of col_ind"
    _assert_equal((torch.from_numpy(offsets).cuda(), torch.from_numpy(out_col).cuda(), torch.from_numpy(eid).cuda()),
                  ref.induced_subgraph_vectorised(row_ptr, col, perm), "the vectorised reference")
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ degenerate lists
def test_degenerate_node_lists(gpu_env):
    import torch
    row_ptr, col, _, _ = ladder()
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int64, row_ptr, col)
    looped = next(v for v in range(LADDER_NODES) if v in col[row_ptr[v]:row_ptr[v + 1]])
    plain = next(v for v in range(16, LADDER_NODES) if v not in col[row_ptr[v]:row_ptr[v + 1]] and row_ptr[v + 1] > row_ptr[v])
    for v in (looped, plain):
        want = ref.induced_subgraph(row_ptr, col, [v])
        assert want[0][-1] == (col[row_ptr[v]:row_ptr[v + 1]] == v).sum() and (want[0][-1] > 0) == (v == looped)
        _assert_equal(g.induced_subgraph(torch.tensor([v], device="cuda"), need_edge_output=True), want, "the single node %d" % v)
    refused = torch.tensor([-1, LADDER_NODES, LADDER_NODES + 5, -7, (1 << 31) - 1, 1 << 40], dtype=torch.int64, device="cuda")
    offsets, out_col, eid = g.induced_subgraph(refused, need_edge_output=True)
    assert offsets.dtype == torch.int32 and offsets.tolist() == [0] * 7 and out_col.numel() == 0 and eid.numel() == 0
    assert out_col.dtype == torch.int32 and eid.dtype == torch.int64
    for dtype in (torch.int32, torch.int64):
        offsets, out_col, eid = g.induced_subgraph(torch.empty(0, dtype=dtype, device="cuda"), need_edge_output=True)
        assert offsets.dtype == torch.int32 and offsets.tolist() == [0]
        assert out_col.dtype == torch.int32 and tuple(out_col.shape) == (0,) and eid.dtype == torch.int64 and tuple(eid.shape) == (0,)
        assert len(g.induced_subgraph(torch.empty(0, dtype=dtype, device="cuda"))) == 2
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ damaged graphs
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_damaged_col_ind_never_matches(gpu_env, col_dtype):
    """col_ind entries of -1, n_nodes = 60 and 2^31 - 1 (the graphs of tests/test_n2v_streams.py), and a node list that
    holds -1 and 60 itself: those values are not members, so no output entry refers to them"""
    import torch
    from test_n2v_streams import small_graphs
    rng = np.random.default_rng(23)
    for name, graph in zip(("sorted", "shuffled"), small_graphs()):
        row_ptr, col = graph[0], graph[1]
        nodes = np.concatenate([[-1, 60], rng.integers(0, 60, 40), [60, -1, 59, 0]]).astype(np.int64)
        want = ref.induced_subgraph(row_ptr, col, nodes)
        assert want[0][-1] >= 40 and {-1, 60, (1 << 31) - 1} <= set(col.tolist())
        g, ts = _structure(gpu_env, "chunked", "cuda", NP_OF[col_dtype], row_ptr, col)
        got = g.induced_subgraph(torch.from_numpy(nodes).cuda(), need_edge_output=True)
        torch.cuda.synchronize()
        _assert_equal(got, want, name)
        out_col, eid = got[1].cpu().numpy(), got[2].cpu().numpy()
        assert ((nodes[out_col] >= 0) & (nodes[out_col] < 60)).all() and np.array_equal(nodes[out_col], col[eid])
        rows = np.diff(got[0].cpu().numpy())
        assert (rows[(nodes < 0) | (nodes >= 60)] == 0).all()
        _destroy(ts)


def test_damaged_row_ptr_gives_empty_rows(gpu_env):
    """five nodes; the pair of node 1 has e < s and the pair of node 3 has e > n_edges: those rows are empty, the others right"""
    import torch
    row_ptr = np.array([0, 3, 2, 5, 9, 7], dtype=np.int64)      # rows: [0, 3), (3, 2) damaged, [2, 5), (5, 9) damaged, (9, 7) damaged
    col = np.array([1, 2, 0, 4, 3, 0, 2], dtype=np.int64)
    nodes = np.array([4, 3, 2, 1, 0, 2], dtype=np.int64)
    want = ref.induced_subgraph(row_ptr, col, nodes)
    assert np.diff(want[0]).tolist() == [0, 0, 3, 0, 3, 3] and want[1].tolist() == [4, 0, 1, 3, 2, 4, 4, 0, 1]
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int64, row_ptr, col)
    _assert_equal(g.induced_subgraph(torch.from_numpy(nodes).cuda(), need_edge_output=True), want, "damaged row_ptr")
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ many rows
@pytest.mark.parametrize("node_dtype,col_dtype", [("int32", "int32"), ("int64", "int64")])
def test_many_rows_equal_the_vectorised_reference(gpu_env, node_dtype, col_dtype):
    """70 001 nodes drawn from [-2, 2002) on the ladder: no multiple of a block, more than one block per CU, every node about
    35 times — first() is taken over many positions; the whole output is compared, and two calls agree"""
    import torch
    row_ptr, col, _, _ = ladder()
    nodes = np.random.default_rng(17).integers(-2, LADDER_NODES + 2, 70001).astype(NP_OF[node_dtype])
    want = ref.induced_subgraph_vectorised(row_ptr, col, nodes)
    assert want[0][-1] >= 500000 and np.unique(want[1]).shape[0] <= LADDER_NODES      # (local ids are first positions only)
    g, ts = _structure(gpu_env, "chunked", "cuda", NP_OF[col_dtype], row_ptr, col)
    dev = torch.from_numpy(nodes).cuda()
    got = g.induced_subgraph(dev, need_edge_output=True)
    _assert_equal(got, want, "70 001 rows")
    again = g.induced_subgraph(dev, need_edge_output=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two calls differ"
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ offset views
@pytest.mark.parametrize("mt,col_dtype", [("continuous", np.int32), ("continuous", np.int64), ("chunked", np.int32),
                                          ("chunked", np.int64)])
def test_graph_tensors_at_odd_storage_offsets(gpu_env, mt, col_dtype):
    """row_ptr a view from element 3 and col_ind a view from element 5 of poisoned arrays (a large negative number, an id that
    is no node), as tests/test_csr_offset_views_gpu.py builds them: an offset dropped or swapped reads the poison"""
    import torch
    import wholegraph_amd.torch as wgth
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, _, starts = ladder()
    roots, views = [], []
    for arr, lead, poison in ((row_ptr, 3, -(1 << 40)), (col.astype(col_dtype), 5, LADDER_NODES + 12345)):
        padded = np.full(lead + arr.shape[0] + 6, poison, dtype=arr.dtype)
        padded[lead:lead + arr.shape[0]] = arr
        root = _wm_array(gpu_env, mt, padded)
        view = root.get_sub_tensor([lead], [lead + arr.shape[0]])
        assert view.storage_offset() == lead and tuple(view.shape) == (arr.shape[0],)
        roots.append(root)
        views.append(view)
    got = wops.induced_subgraph(views[0].wmb_tensor, views[1].wmb_tensor, torch.from_numpy(np.array(starts)).cuda(),
                                need_edge_output=True)
    _assert_equal(got, ref.ladder_subgraph(), "offset views, %s" % mt)
    for t in views + roots:
        wgth.destroy_wholememory_tensor(t)


# ------------------------------------------------------------------------------------------------ overflow
def test_a_subgraph_of_2e9_entries_is_refused_after_the_count(gpu_env, monkeypatch):
    """two nodes, node 0 with 40 000 entries that all say 1; nodes = 60 000 times node 0, then node 1: m = 2.4e9. The int32 scan
    cannot see that, the 64-bit total beside it does: INVALID_INPUT, no output allocated, and the next call works.
    (The count pass alone runs: 2.4e9 probes of a two-key table.)"""
    import time
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd import binding
    from wholegraph_amd.torch import wholegraph_env
    row_ptr = np.array([0, 40000, 40000], dtype=np.int64)
    col = np.ones(40000, dtype=np.int32)
    g, ts = _structure(gpu_env, "continuous", "cuda", np.int32, row_ptr, col)
    nodes = torch.cat([torch.zeros(60000, dtype=torch.int32), torch.ones(1, dtype=torch.int32)]).cuda()
    allocated = []      # what the library asked the output contexts of the call for

    class Recording(wholegraph_env.TorchMemoryContext):
        def set_tensor(self, t):
            if t is not None:
                allocated.append(tuple(t.shape))
            super().set_tensor(t)
    monkeypatch.setattr(wops, "TorchMemoryContext", Recording)
    t0 = time.perf_counter()
    with pytest.raises(binding.WholeMemoryError) as e:
        g.induced_subgraph(nodes, need_edge_output=True)
    torch.cuda.synchronize()
    print("the refused call took %.3f s" % (time.perf_counter() - t0))
    assert e.value.code == 6       # WHOLEMEMORY_INVALID_INPUT
    assert allocated == [], "outputs were allocated for a refused call: %s" % allocated
    small = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    offsets, out_col, eid = g.induced_subgraph(small, need_edge_output=True)
    assert offsets.tolist() == [0, 40000, 40000, 80000] and (out_col == 1).all()
    assert torch.equal(eid, torch.arange(40000, device="cuda").repeat(2))
    assert allocated == [(80000,), (80000,)]      # (the recorder does see a call's allocations)
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ plain tensors, DISTRIBUTED
def test_plain_device_tensors(gpu_env):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    row_ptr, col, _, starts = ladder()
    hold = [torch.from_numpy(np.array(a)).cuda() for a in (row_ptr, col.astype(np.int32))]
    wr, wc = [wrap_torch_tensor(t) for t in hold]
    got = wops.induced_subgraph(wr.handle, wc.handle, torch.from_numpy(starts.astype(np.int32)).cuda(), need_edge_output=True)
    _assert_equal(got, ref.ladder_subgraph(), "plain device tensors")


def test_distributed_csr_is_not_implemented(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    row_ptr, col, _, starts = ladder()
    nodes = torch.from_numpy(np.array(starts)).cuda()
    g, ts = _structure(gpu_env, "distributed", "cuda", np.int64, row_ptr, col)
    with pytest.raises(binding.WholeMemoryError) as e:
        g.induced_subgraph(nodes)
    assert e.value.code == 2 and isinstance(e.value, NotImplementedError)      # WHOLEMEMORY_NOT_IMPLEMENTED
    _destroy(ts)
    ts = [_wm_array(gpu_env, "chunked", row_ptr), _wm_array(gpu_env, "distributed", col)]      # col_ind alone
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    with pytest.raises(binding.WholeMemoryError) as e:
        g.induced_subgraph(nodes, need_edge_output=True)
    assert e.value.code == 2
    _destroy(ts)
