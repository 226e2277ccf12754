"""Every op that reads the WholeMemory CSR graph, on graph tensors whose storage offset is not 0 (MI355X).

The graph arrays are 1-D sub-tensor views of larger WholeMemory arrays: csr_row_ptr starts at element 3, csr_col_ptr at
element 5 (an int32 view starts 20 bytes in: neither 8- nor 16-byte aligned), the edge weights at element 7 and an edge
attribute at element 9 — odd and mutually different, so that an offset that is dropped, or taken from another array, reads
the padding or shifted data. The padding before and behind every view holds poison that cannot pass for data: a large negative
number in csr_row_ptr, an id >= n_nodes in csr_col_ptr, a huge weight, an attribute no edge has. CONTINUOUS and CHUNKED (where
the offset meets the chunk arithmetic), int32 and int64 columns.

The graph is the degree ladder of tests/test_sampler_edges_gpu.py, which reaches every sampler kernel class. Every reference
is fed the unpadded arrays and every comparison is exact: the samplers against the oracle (edge ids are positions in the
view), the walks, node2vec walks and negatives against their Python restatements, the fused hop and the chain against the
two-op sequence on the same views, the chain's edge attribute against the attribute array at the returned edge ids."""
import numpy as np
import pytest

import _n2v_ref as n2v_ref
import _neg_ref as neg_ref
import _walk_ref as walk_ref
from test_sampler_edges_gpu import (ladder_graph, ladder_weights, unweighted_reference, unweighted_seed, weighted_reference,
                                    weighted_seed)

pytestmark = pytest.mark.gpu

ROW_AT, COL_AT, WEIGHT_AT, ATTR_AT, BEHIND = 3, 5, 7, 9, 6      # elements before each view, and behind every one
UNWEIGHTED_FANOUTS = (-1, 1, 33, 65, 1024, 1025)      # all neighbours, the two register kernels, LDS (twice), reservoir
WEIGHTED_FANOUTS = (1, 33, 65, 257, 1024)             # the two register kernels, the list with 128 and with 256 threads
HOP_FANOUTS = (30, 65)
BATCH, STEPS, NEGATIVES, TRIES = 64, 5, 5, 8
WALK_SEED, N2V_PQ = 4321, (0.25, 4.0)

CASES = pytest.mark.parametrize("mt,col_dtype", [("continuous", np.int32), ("continuous", np.int64), ("chunked", np.int32),
                                                 ("chunked", np.int64)])
_CACHE = {}


def graph(in_order=False):
    """-> row_ptr int64, col int64, weights float32, attribute int64 (read-only, shared): the ladder with the `ordinary`
    weights and edge position * 3 + 1 as the attribute, or its copy with every row ascending (weights and attribute moved
    with the columns)"""
    if in_order not in _CACHE:
        row_ptr, col, _ = ladder_graph()
        weights = ladder_weights("ordinary", col.shape[0])
        attr = np.arange(col.shape[0], dtype=np.int64) * 3 + 1
        if in_order:
            col, weights, attr = np.array(col), np.array(weights), np.array(attr)
            for v in range(row_ptr.shape[0] - 1):
                s, e = int(row_ptr[v]), int(row_ptr[v + 1])
                o = np.argsort(col[s:e], kind="stable")
                col[s:e], weights[s:e], attr[s:e] = col[s:e][o], weights[s:e][o], attr[s:e][o]
        for a in (col, weights, attr):
            a.setflags(write=False)
        _CACHE[in_order] = (row_ptr, col, weights, attr)
    return _CACHE[in_order]


def batch():
    """64 nodes of the ladder, the first two not nodes at all"""
    nodes = np.array(ladder_graph()[2][:BATCH])
    nodes[0], nodes[1] = -1, ladder_graph()[0].shape[0] - 1
    return nodes


def reference(name, compute):
    if name not in _CACHE:
        _CACHE[name] = compute()
    return _CACHE[name]


class Views:
    """the four graph arrays as views into poisoned WholeMemory arrays; .row / .col / .weight / .attr are the handles"""

    def __init__(self, comm, mt, col_dtype, in_order=False):
        from test_weighted_chain_gpu import _wm_array
        row_ptr, col, weights, attr = graph(in_order)
        n_nodes = row_ptr.shape[0] - 1
        self.roots, self.views = [], []
        for arr, lead, poison in ((row_ptr, ROW_AT, -(1 << 40)), (col.astype(col_dtype), COL_AT, n_nodes + 12345),
                                  (weights, WEIGHT_AT, 3e38), (attr, ATTR_AT, -7)):
            padded = np.full(lead + arr.shape[0] + BEHIND, poison, dtype=arr.dtype)
            padded[lead:lead + arr.shape[0]] = arr
            root = _wm_array(comm, mt, padded)
            view = root.get_sub_tensor([lead], [lead + arr.shape[0]])
            assert view.storage_offset() == lead and tuple(view.shape) == (arr.shape[0],)
            self.roots.append(root)
            self.views.append(view)
        self.row, self.col, self.weight, self.attr = [v.wmb_tensor for v in self.views]

    def destroy(self):
        import wholegraph_amd.torch as wgth
        for t in self.views + self.roots:
            wgth.destroy_wholememory_tensor(t)


def _equal(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and np.array_equal(got, want), what


@CASES
def test_samplers_equal_the_oracle(gpu_env, mt, col_dtype):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    v = Views(gpu_env, mt, col_dtype)
    centers = torch.from_numpy(ladder_graph()[2].astype(col_dtype)).cuda()
    runs = [(m, unweighted_seed(m), unweighted_reference(m), None) for m in UNWEIGHTED_FANOUTS]
    runs += [(m, weighted_seed(m), weighted_reference("ordinary", m), v.weight) for m in WEIGHTED_FANOUTS]
    for m, seed, (o_off, o_ids, o_lid, o_egid), weight in runs:
        what = "%s, max_sample_count=%d" % ("unweighted" if weight is None else "weighted", m)
        if weight is None:
            got = wops.unweighted_sample_without_replacement(v.row, v.col, centers, m, seed, True, True)
        else:
            got = wops.weighted_sample_without_replacement(v.row, v.col, weight, centers, m, seed, True, True)
        off, ids, lid, egid = got
        _equal(off, o_off, "offsets: " + what)
        _equal(egid, o_egid, "edge ids: " + what)
        _equal(ids, o_ids.astype(col_dtype), "ids: " + what)
        _equal(lid, o_lid, "centre local ids: " + what)
    v.destroy()


@CASES
def test_walks_equal_the_reference(gpu_env, mt, col_dtype):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, weights, _ = graph()
    starts = batch()
    v = Views(gpu_env, mt, col_dtype)
    dev_starts = torch.from_numpy(starts).cuda()
    uniform = reference("uniform walks", lambda: walk_ref.uniform_walks(row_ptr, col, starts, STEPS, WALK_SEED))
    weighted = reference("weighted walks", lambda: walk_ref.weighted_walks(row_ptr, col, weights, starts, STEPS, WALK_SEED))
    assert (uniform[1] >= 0).sum() >= 2 * BATCH and (weighted[1] >= 0).sum() >= 2 * BATCH
    for want, weight in ((uniform, None), (weighted, v.weight)):
        walks, eids = wops.random_walk(v.row, v.col, dev_starts, STEPS, WALK_SEED, wm_csr_weight_ptr_tensor=weight,
                                       need_edge_output=True)
        what = "uniform" if weight is None else "weighted"
        _equal(walks, want[0].astype(col_dtype), "walks: " + what)
        _equal(eids, want[1], "edge ids: " + what)
    v.destroy()


@CASES
@pytest.mark.parametrize("in_order", [False, True], ids=["unsorted", "sorted"])
def test_node2vec_walks_equal_the_reference(gpu_env, mt, col_dtype, in_order):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, weights, _ = graph(in_order)
    starts = batch()
    p, q = N2V_PQ
    want = reference(("node2vec", in_order),
                     lambda: n2v_ref.node2vec_walks(row_ptr, col, weights, starts, STEPS, p, q, WALK_SEED))
    assert (want[1] >= 0).sum() >= 2 * BATCH
    v = Views(gpu_env, mt, col_dtype, in_order)
    walks, eids = wops.node2vec_walk(v.row, v.col, torch.from_numpy(starts).cuda(), STEPS, p, q, WALK_SEED,
                                     wm_csr_weight_ptr_tensor=v.weight, col_sorted=in_order, need_edge_output=True)
    _equal(walks, want[0].astype(col_dtype), "walks")
    _equal(eids, want[1], "edge ids")
    v.destroy()


@CASES
@pytest.mark.parametrize("in_order", [False, True], ids=["unsorted", "sorted"])
def test_negatives_equal_the_reference(gpu_env, mt, col_dtype, in_order):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, _, _ = graph(in_order)
    src = batch()
    v = Views(gpu_env, mt, col_dtype, in_order)
    for mode_name, mode in sorted(wops.NEGATIVE_MODES.items()):
        want = reference(("negatives", in_order, mode),
                         lambda: neg_ref.negative_samples(row_ptr, col, src, NEGATIVES, mode, 3, TRIES, WALK_SEED))
        assert (want >= 0).sum() >= 2 * BATCH
        got = wops.negative_sample(v.row, v.col, torch.from_numpy(src).cuda(), NEGATIVES, WALK_SEED, mode=mode_name,
                                   max_tries=TRIES, col_sorted=in_order)
        _equal(got, want.astype(col_dtype), "negatives, mode %s" % mode_name)
    v.destroy()


def _two_ops(v, weight, frontier, m, seed):
    """sampler + append_unique on the same views -> offsets, unique, neighbor_pos, center_lid, edge ids"""
    import wholegraph_amd.torch.graph_ops as gops
    import wholegraph_amd.torch.wholegraph_ops as wops
    if weight is None:
        off, ids, lid, egid = wops.unweighted_sample_without_replacement(v.row, v.col, frontier, m, seed, True, True)
    else:
        off, ids, lid, egid = wops.weighted_sample_without_replacement(v.row, v.col, weight, frontier, m, seed, True, True)
    uniq, pos = gops.append_unique(frontier, ids, need_neighbor_raw_to_unique=True)
    return off, uniq, pos, lid, egid


def _assert_hop(got, want, what):
    import torch
    for name, a, b in zip(("offsets", "unique", "neighbor_pos", "center_lid", "edge ids"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), "%s: %s" % (name, what)


@CASES
def test_fused_hop_equals_the_two_ops(gpu_env, mt, col_dtype):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    v = Views(gpu_env, mt, col_dtype)
    frontier = torch.from_numpy(ladder_graph()[2].astype(col_dtype)).cuda()
    for weight in (None, v.weight):
        for m in HOP_FANOUTS:
            what = "%s, max_sample_count=%d" % ("unweighted" if weight is None else "weighted", m)
            fused = wops.sample_append_unique(v.row, v.col, frontier, m, 77 + m, wm_csr_weight_ptr_tensor=weight,
                                              need_edge_output=True)
            assert fused is not None, "the fused hop was declined: " + what
            _assert_hop(fused, _two_ops(v, weight, frontier, m, 77 + m), what)
    v.destroy()


@CASES
def test_chain_equals_the_two_ops(gpu_env, mt, col_dtype):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    attr = torch.from_numpy(np.array(graph()[3])).cuda()
    v = Views(gpu_env, mt, col_dtype)
    seeds = torch.from_numpy(ladder_graph()[2][:101].astype(col_dtype)).cuda()
    for weight in (None, v.weight):
        for m in HOP_FANOUTS:
            what = "%s, max_sample_count=%d" % ("unweighted" if weight is None else "weighted", m)
            hop_seeds = [91 + m, 102 + m]
            chain = wops.multilayer_sample(v.row, v.col, seeds, [m, m], hop_seeds, wm_csr_weight_ptr_tensor=weight,
                                           wm_edge_attr_tensors=[v.attr])
            assert chain is not None, "the chain was declined: " + what
            torch.cuda.synchronize()
            frontier = seeds
            for h, hop in enumerate(chain):
                want = _two_ops(v, weight, frontier, m, hop_seeds[h])
                _assert_hop(hop[:4] + (hop[5],), want, "hop %d, %s" % (h, what))
                assert len(hop[6]) == 1 and hop[6][0].dtype == attr.dtype, what
                assert torch.equal(hop[6][0], attr[hop[5]]), "edge attribute: hop %d, %s" % (h, what)
                frontier = want[1]
    v.destroy()
