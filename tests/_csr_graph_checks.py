"""What tests/test_csr_offset_views_gpu.py (one rank, sub-tensor views) and tests/test_csr_graph_ranks_gpu.py with its worker
tests/_csr_ranks_worker.py (the graph split over several ranks) share: the ladder graph with weights and an edge attribute, the
graph as WholeMemory tensors in any layout, and one check per op that reads the WholeMemory CSR graph.

The graph is the degree ladder of tests/test_sampler_edges_gpu.py, which reaches every sampler kernel class. Every reference is
fed the full, unpadded, unsplit arrays and every comparison is exact: the samplers against the oracle, the walks, node2vec
walks, negatives and the induced subgraph against their Python restatements, the fused hop and the chain against the two-op
sequence on the same handles, the chain's edge attribute against the attribute array at the returned edge ids. A check takes
the graph's handles, the dtype of csr_col_ptr, the caller's batch of node ids and `seed`, which is added to every seed the
check uses (0 on one rank; the rank's number in the worker, so that each rank has references of its own). References are
computed once per (op, batch, seed) and shared by the layouts.

Also the entry partitions of the custom-partition layouts (custom_partitions), which need no GPU."""
import numpy as np

import _isub_ref as isub_ref
import _n2v_ref as n2v_ref
import _neg_ref as neg_ref
import _walk_ref as walk_ref
import oracle
from test_sampler_edges_gpu import (assert_no_nan_keys, ladder_graph, ladder_weights, unweighted_seed, weighted_seed)

ROW_AT, COL_AT, WEIGHT_AT, ATTR_AT, BEHIND = 3, 5, 7, 9, 6      # elements before each view, and behind every one
UNWEIGHTED_FANOUTS = (-1, 1, 33, 65, 1024, 1025)      # all neighbours, the two register kernels, LDS (twice), reservoir
WEIGHTED_FANOUTS = (1, 33, 65, 257, 1024)             # the two register kernels, the list with 128 and with 256 threads
HOP_FANOUTS = (30, 65)
BATCH, STEPS, NEGATIVES, TRIES = 64, 5, 5, 8
WALK_SEED, N2V_PQ = 4321, (0.25, 4.0)
HUB_DEGREE = 16385

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


def hub_node():
    row_ptr = ladder_graph()[0]
    hub = int(np.argmax(np.diff(row_ptr)))
    assert row_ptr[hub + 1] - row_ptr[hub] == HUB_DEGREE
    return hub


def reference(name, compute):
    if name not in _CACHE:
        _CACHE[name] = compute()
    return _CACHE[name]


def references_made_by(compute, *args):
    """-> what compute(*args) adds to the shared references; a forked child computes, its parent adopts (adopt_references)"""
    before = set(_CACHE)
    compute(*args)
    return {name: value for name, value in _CACHE.items() if name not in before}


def adopt_references(made):
    _CACHE.update(made)


def _ids(nodes):
    """a batch as part of a reference's name"""
    return np.asarray(nodes).astype(np.int64).tobytes()


# ------------------------------------------------------------------------------------------------ the custom partitions
def searches(partition):
    """does gref_load look the owner up in the rank offsets? It divides by the first rank's size instead when every rank but
    the last holds exactly that and the last no more (plan_partition, csrc/memory_handle.cpp)."""
    return not (partition[-1] <= partition[0] and all(p == partition[0] for p in partition[:-1]))


def custom_partitions(world, cut, middle=0):
    """The entry partitions of the custom-partition layout for 2 or 3 ranks -> {"row": of csr_row_ptr, "edge": of csr_col_ptr,
    the weights and the attribute, "row_node": v, "edge_node": x}.
    csr_row_ptr is cut between row_ptr[v] and row_ptr[v + 1] of a node v of batch(): s is read from one rank and e from the
    next. The edge arrays are cut strictly inside the row of node x: the hub (cut "hub") or a node of batch() of degree
    3 .. 32 (cut "short"). Three ranks: the middle rank holds `middle` entries (0, or 1 where an empty partition is refused),
    taken from behind the cut, and both of its ends lie inside the same row. Every first partition is the smaller one, so that
    two ranks search too."""
    assert world in (2, 3) and cut in ("hub", "short") and middle in (0, 1)
    row_ptr = ladder_graph()[0]
    n_nodes, n_edges = row_ptr.shape[0] - 1, int(row_ptr[-1])
    deg = np.diff(row_ptr)
    nodes = [int(v) for v in batch() if 0 <= v < n_nodes]
    mid = [] if world == 2 else [middle]
    v = max((v for v in nodes if 2 * (v + 1) < n_nodes + 1), key=lambda v: int(deg[v]))
    row = [v + 1] + mid + [n_nodes + 1 - (v + 1) - sum(mid)]
    if cut == "hub":
        x = hub_node()
    else:
        x = min((v for v in nodes if 3 <= deg[v] <= 32), key=lambda v: int(row_ptr[v]))
    a = int(row_ptr[x]) + int(deg[x]) // 2
    edge = [a] + mid + [n_edges - a - sum(mid)]
    return {"row": row, "edge": edge, "row_node": v, "edge_node": x}


def owner_of(partition, entry):
    """the rank gref_load's search finds for an entry: the last one whose first entry is not behind it"""
    starts = np.concatenate([[0], np.cumsum(partition)])[:-1]
    return max(r for r in range(len(partition)) if starts[r] <= entry)


def assert_custom_partitions(world, cut, middle=0):
    """the cuts of custom_partitions fall where its docstring says (host only) -> the partitions"""
    p = custom_partitions(world, cut, middle)
    row_ptr = ladder_graph()[0]
    n_nodes, n_edges = row_ptr.shape[0] - 1, int(row_ptr[-1])
    members = set(int(v) for v in batch())
    v, x = p["row_node"], p["edge_node"]
    # csr_row_ptr: s = row_ptr[v] on rank 0, e = row_ptr[v + 1] on the next rank that holds anything
    assert v in members and 0 <= v < n_nodes and row_ptr[v + 1] > row_ptr[v], v
    assert owner_of(p["row"], v) == 0 and owner_of(p["row"], v + 1) == (1 if world == 2 or middle else 2), p["row"]
    # the edge arrays: every cut strictly inside the row of x
    s, e = int(row_ptr[x]), int(row_ptr[x + 1])
    if cut == "hub":
        assert e - s == HUB_DEGREE
    else:
        assert x in members and 2 <= e - s <= 32, (x, e - s)
    cuts = np.cumsum(p["edge"])[:-1]
    assert all(s < c < e for c in cuts), (cuts, s, e)
    assert owner_of(p["edge"], s) == 0 and owner_of(p["edge"], e - 1) == world - 1, p["edge"]
    assert sum(p["row"]) == n_nodes + 1 and sum(p["edge"]) == n_edges
    for part in (p["row"], p["edge"]):
        assert len(part) == world and len(set(part)) > 1 and searches(part), part
        assert world == 2 or part[1] == middle, part
    return p


# ------------------------------------------------------------------------------------------------ the graph in WholeMemory
def wm_array(comm, mt, arr, loc="cuda", entries=None):
    """a 1-D WholeMemory tensor holding `arr`, every rank filling its own part (collective)"""
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, mt, loc, [arr.shape[0]], torch.from_numpy(arr).dtype, [1], entries)
    local, start = t.get_local_tensor(host_view=(loc == "cpu"))
    local.copy_(torch.from_numpy(arr[start:start + local.shape[0]]))
    torch.cuda.synchronize()
    return t


class Graph:
    """the four graph arrays as WholeMemory tensors: .tensors are csr_row_ptr, csr_col_ptr, the weights and the attribute,
    .row / .col / .weight / .attr their handles. as_views: each is a sub-tensor view into a larger array whose padding holds
    poison that cannot pass for data (a large negative number in csr_row_ptr, an id >= n_nodes in csr_col_ptr, a huge weight,
    an attribute no edge has). entries: {"row": ..., "edge": ...}, the entry partitions of custom_partitions."""

    def __init__(self, comm, mt, col_dtype, in_order=False, loc="cuda", entries=None, as_views=False):
        row_ptr, col, weights, attr = graph(in_order)
        n_nodes = row_ptr.shape[0] - 1
        self.in_order, self.roots, self.tensors = in_order, [], []
        for arr, lead, poison, part in ((row_ptr, ROW_AT, -(1 << 40), "row"), (col.astype(col_dtype), COL_AT, n_nodes + 12345, "edge"),
                                        (weights, WEIGHT_AT, 3e38, "edge"), (attr, ATTR_AT, -7, "edge")):
            if not as_views:
                self.tensors.append(wm_array(comm, mt, np.array(arr), loc, None if entries is None else entries[part]))
                continue
            padded = np.full(lead + arr.shape[0] + BEHIND, poison, dtype=arr.dtype)
            padded[lead:lead + arr.shape[0]] = arr
            root = wm_array(comm, mt, padded, loc)
            view = root.get_sub_tensor([lead], [lead + arr.shape[0]])
            assert view.storage_offset() == lead and tuple(view.shape) == (arr.shape[0],)
            self.roots.append(root)
            self.tensors.append(view)
        self.row, self.col, self.weight, self.attr = [t.wmb_tensor for t in self.tensors]

    def structure(self):
        """-> GraphStructure with the weights as edge attribute "w" and the attribute as "a" """
        import wholegraph_amd.torch as wgth
        g = wgth.GraphStructure()
        g.set_csr_graph(self.tensors[0], self.tensors[1])
        g.set_edge_attribute("w", self.tensors[2])
        g.set_edge_attribute("a", self.tensors[3])
        return g

    def destroy(self):
        import wholegraph_amd.torch as wgth
        for t in self.tensors + self.roots:      # (views before the arrays they look into)
            wgth.destroy_wholememory_tensor(t)


def Views(comm, mt, col_dtype, in_order=False):
    """the graph as sub-tensor views: csr_row_ptr starts at element 3, csr_col_ptr at element 5, the weights at element 7 and
    the attribute at element 9 of poisoned arrays"""
    return Graph(comm, mt, col_dtype, in_order, as_views=True)


def _equal(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _dev(nodes, dtype=None):
    import torch
    return torch.from_numpy(np.array(nodes if dtype is None else np.asarray(nodes).astype(dtype))).cuda()


# ------------------------------------------------------------------------------------------------ the one-hop samplers
def unweighted_reference(centers, m, seed):
    row_ptr, col, _, _ = graph()
    c = np.asarray(centers).astype(np.int64)
    return reference(("unweighted", m, seed, _ids(c)), lambda: oracle.sample_unweighted(row_ptr, col, c, m, unweighted_seed(m) + seed))


def weighted_reference(centers, m, seed):
    row_ptr, col, weights, _ = graph()
    c = np.asarray(centers).astype(np.int64)

    def compute():
        assert_no_nan_keys(row_ptr, c, weights, m, weighted_seed(m) + seed)
        return oracle.sample_weighted(row_ptr, col, weights, c, m, weighted_seed(m) + seed)
    return reference(("weighted", m, seed, _ids(c)), compute)


def check_samplers(h, col_dtype, centers, seed, unweighted=UNWEIGHTED_FANOUTS, weighted=WEIGHTED_FANOUTS):
    """both samplers with centre-local and edge outputs: offsets, ids (cast to the column dtype), local ids and edge ids"""
    import wholegraph_amd.torch.wholegraph_ops as wops
    dev_centers = _dev(centers)
    runs = [(m, unweighted_seed(m) + seed, unweighted_reference(centers, m, seed), None) for m in unweighted]
    runs += [(m, weighted_seed(m) + seed, weighted_reference(centers, m, seed), h.weight) for m in weighted]
    for m, op_seed, (o_off, o_ids, o_lid, o_egid), weight in runs:
        what = "%s, max_sample_count=%d" % ("unweighted" if weight is None else "weighted", m)
        if weight is None:
            got = wops.unweighted_sample_without_replacement(h.row, h.col, dev_centers, m, op_seed, True, True)
        else:
            got = wops.weighted_sample_without_replacement(h.row, h.col, weight, dev_centers, m, op_seed, True, True)
        off, ids, lid, egid = got
        _equal(off, o_off, "offsets: " + what)
        _equal(egid, o_egid, "edge ids: " + what)
        _equal(ids, o_ids.astype(col_dtype), "ids: " + what)
        _equal(lid, o_lid, "centre local ids: " + what)


# ------------------------------------------------------------------------------------------------ walks
def walk_references(starts, seed):
    """-> (uniform, weighted): each (walks, edge ids) of tests/_walk_ref.py on the full arrays"""
    row_ptr, col, weights, _ = graph()
    s, walk_seed = np.asarray(starts).astype(np.int64), WALK_SEED + seed
    uniform = reference(("uniform walks", seed, _ids(s)), lambda: walk_ref.uniform_walks(row_ptr, col, s, STEPS, walk_seed))
    weighted = reference(("weighted walks", seed, _ids(s)),
                         lambda: walk_ref.weighted_walks(row_ptr, col, weights, s, STEPS, walk_seed))
    return uniform, weighted


def _assert_real_steps(eids, n):
    """the reference walks take at least 2 * BATCH steps (of a full batch): the case cannot pass on walks that all end at once"""
    assert n == 0 or (n >= BATCH and (eids >= 0).sum() >= 2 * BATCH)


def check_walks(h, col_dtype, starts, seed):
    import wholegraph_amd.torch.wholegraph_ops as wops
    uniform, weighted = walk_references(starts, seed)
    _assert_real_steps(uniform[1], len(starts))
    _assert_real_steps(weighted[1], len(starts))
    dev_starts = _dev(starts)
    for want, weight in ((uniform, None), (weighted, h.weight)):
        walks, eids = wops.random_walk(h.row, h.col, dev_starts, STEPS, WALK_SEED + seed, wm_csr_weight_ptr_tensor=weight,
                                       need_edge_output=True)
        what = "uniform" if weight is None else "weighted"
        _equal(walks, want[0].astype(col_dtype), "walks: " + what)
        _equal(eids, want[1], "edge ids: " + what)


def node2vec_reference(in_order, starts, seed):
    """-> (walks, edge ids) of tests/_n2v_ref.py with the weights, on the ladder or on its copy with ascending rows"""
    row_ptr, col, weights, _ = graph(in_order)
    p, q = N2V_PQ
    s = np.asarray(starts).astype(np.int64)
    return reference(("node2vec", in_order, seed, _ids(s)),
                     lambda: n2v_ref.node2vec_walks(row_ptr, col, weights, s, STEPS, p, q, WALK_SEED + seed))


def check_node2vec(h, col_dtype, starts, seed):
    """weighted node2vec walks; the graph's rows are ascending (h.in_order) or not, and col_sorted says so"""
    import wholegraph_amd.torch.wholegraph_ops as wops
    p, q = N2V_PQ
    want = node2vec_reference(h.in_order, starts, seed)
    _assert_real_steps(want[1], len(starts))
    walks, eids = wops.node2vec_walk(h.row, h.col, _dev(starts), STEPS, p, q, WALK_SEED + seed, wm_csr_weight_ptr_tensor=h.weight,
                                     col_sorted=h.in_order, need_edge_output=True)
    _equal(walks, want[0].astype(col_dtype), "walks")
    _equal(eids, want[1], "edge ids")


# ------------------------------------------------------------------------------------------------ negatives
def check_negatives(h, col_dtype, src, seed):
    """every mode of NEGATIVE_MODES; the graph's rows are ascending (h.in_order) or not, and col_sorted says so"""
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, _, _ = graph(h.in_order)
    s = np.asarray(src).astype(np.int64)
    for mode_name, mode in sorted(wops.NEGATIVE_MODES.items()):
        want = reference(("negatives", h.in_order, mode, seed, _ids(s)),
                         lambda: neg_ref.negative_samples(row_ptr, col, s, NEGATIVES, mode, 3, TRIES, WALK_SEED + seed))
        assert len(src) == 0 or (len(src) >= BATCH and (want >= 0).sum() >= 2 * BATCH)
        got = wops.negative_sample(h.row, h.col, _dev(src), NEGATIVES, WALK_SEED + seed, mode=mode_name, max_tries=TRIES,
                                   col_sorted=h.in_order)
        _equal(got, want.astype(col_dtype), "negatives, mode %s" % mode_name)


# ------------------------------------------------------------------------------------------------ subgraphs
def check_induced_subgraph(h, col_dtype, nodes):
    """with edge ids: offsets, local columns and edge ids against tests/_isub_ref.py"""
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, _, _ = graph()
    want = reference(("induced subgraph", _ids(nodes)), lambda: isub_ref.induced_subgraph(row_ptr, col, np.asarray(nodes)))
    got = wops.induced_subgraph(h.row, h.col, _dev(nodes), need_edge_output=True)
    assert len(got) == 3
    for name, a, b in zip(("offsets", "col", "edge ids"), got, want):
        _equal(a, b, "induced subgraph: " + name)


def check_saint(h, col_dtype, roots, seed):
    """saint_random_walk_subgraph = walks of the reference -> sorted distinct nodes -> the reference's induced subgraph"""
    row_ptr, col, _, _ = graph()
    g = h.structure()
    for (walks, _), weight_name in zip(walk_references(roots, seed), (None, "w")):
        nodes = np.unique(walks[walks >= 0])
        want = (nodes.astype(col_dtype),) + reference(("induced subgraph", _ids(nodes)),
                                                       lambda: isub_ref.induced_subgraph(row_ptr, col, nodes))
        got = g.saint_random_walk_subgraph(_dev(roots), STEPS, random_seed=WALK_SEED + seed, weight_name=weight_name,
                                           need_edge_output=True)
        assert len(got) == 4
        for name, a, b in zip(("nodes", "offsets", "col", "edge ids"), got, want):
            _equal(a, b, "saint, %s: %s" % ("uniform" if weight_name is None else "weighted", name))


# ------------------------------------------------------------------------------------------------ the fused hop and the chain
def _two_ops(h, weight, frontier, m, seed):
    """sampler + append_unique on the same handles -> offsets, unique, neighbor_pos, center_lid, edge ids"""
    import wholegraph_amd.torch.graph_ops as gops
    import wholegraph_amd.torch.wholegraph_ops as wops
    if weight is None:
        off, ids, lid, egid = wops.unweighted_sample_without_replacement(h.row, h.col, frontier, m, seed, True, True)
    else:
        off, ids, lid, egid = wops.weighted_sample_without_replacement(h.row, h.col, weight, frontier, m, seed, True, True)
    uniq, pos = gops.append_unique(frontier, ids, need_neighbor_raw_to_unique=True)
    return off, uniq, pos, lid, egid


def _assert_hop(got, want, what):
    import torch
    for name, a, b in zip(("offsets", "unique", "neighbor_pos", "center_lid", "edge ids"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), "%s: %s" % (name, what)


def check_fused_hop(h, col_dtype, frontier, seed, may_decline=False):
    """sample_append_unique, unweighted and weighted, is taken and equals the two ops. The frontier is cast to the column dtype
    (the fused hop declines other ids); an empty frontier is declined. may_decline (a DISTRIBUTED graph, whose sampler is a
    collective): the two ops run on every rank whatever the hop answers, and a hop that is taken equals them.
    -> how many of the hops were taken"""
    import wholegraph_amd.torch.wholegraph_ops as wops
    frontier = _dev(frontier, col_dtype)
    taken = 0
    for weight in (None, h.weight):
        for m in HOP_FANOUTS:
            what = "%s, max_sample_count=%d" % ("unweighted" if weight is None else "weighted", m)
            fused = wops.sample_append_unique(h.row, h.col, frontier, m, 77 + m + seed, wm_csr_weight_ptr_tensor=weight,
                                              need_edge_output=True)
            if frontier.shape[0] == 0:
                assert fused is None, "the fused hop took an empty frontier: " + what
            elif not may_decline:
                assert fused is not None, "the fused hop was declined: " + what
            if fused is not None or may_decline:
                want = _two_ops(h, weight, frontier, m, 77 + m + seed)
                if fused is not None:
                    _assert_hop(fused, want, what)
                    taken += 1
    return taken


def check_chain(h, col_dtype, seeds, seed, may_decline=False):
    """multilayer_sample([m, m]) with the attribute: hop by hop equals the two ops, its attribute equals attr[edge ids].
    Empty seeds are declined; may_decline as in check_fused_hop. -> how many of the chains were taken"""
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    attr = _dev(graph()[3])
    seeds = _dev(seeds, col_dtype)
    taken = 0
    for weight in (None, h.weight):
        for m in HOP_FANOUTS:
            what = "%s, max_sample_count=%d" % ("unweighted" if weight is None else "weighted", m)
            hop_seeds = [91 + m + seed, 102 + m + seed]
            chain = wops.multilayer_sample(h.row, h.col, seeds, [m, m], hop_seeds, wm_csr_weight_ptr_tensor=weight,
                                           wm_edge_attr_tensors=[h.attr])
            if seeds.shape[0] == 0:
                assert chain is None, "the chain took empty seeds: " + what
            elif not may_decline:
                assert chain is not None, "the chain was declined: " + what
            if chain is None and not may_decline:
                continue
            torch.cuda.synchronize()
            taken += chain is not None
            frontier = seeds
            for hop in range(2):
                want = _two_ops(h, weight, frontier, m, hop_seeds[hop])
                if chain is not None:
                    got = chain[hop]
                    _assert_hop(got[:4] + (got[5],), want, "hop %d, %s" % (hop, what))
                    assert len(got[6]) == 1 and got[6][0].dtype == attr.dtype, what
                    assert torch.equal(got[6][0], attr[got[5]]), "edge attribute: hop %d, %s" % (hop, what)
                frontier = want[1]
    return taken


def check_deferred_chain(comm, h, col_dtype, seeds, seed):
    """The chain's deferred form (GraphStructure.multilayer_sample_begin with edge attributes) feeds a gather of a CHUNKED
    table before the host has waited; its lists equal the eager chain's, the padded frontier is the outermost frontier followed
    by -1 and the gather filled exactly its rows. Collective (the table); a rank with empty seeds only builds the table."""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding
    n_nodes, dim = graph()[0].shape[0] - 1, 32
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [n_nodes, dim])
    local, start = emb.get_embedding_tensor().get_local_tensor()
    rows = torch.arange(start, start + local.shape[0], device="cuda", dtype=torch.float32)
    local.copy_(rows.unsqueeze(1) + torch.arange(dim, device="cuda") / 64.0)
    torch.cuda.synchronize()
    comm.barrier()
    g = h.structure()
    seeds = _dev(seeds, col_dtype)
    names = ["a", "__edge_id__", "w"]
    for weight_name in ((None, "w") if seeds.shape[0] else ()):
        for m in HOP_FANOUTS:
            what = "deferred, %s, max_sample_count=%d" % ("unweighted" if weight_name is None else "weighted", m)
            hop_seeds = [91 + m + seed, 102 + m + seed]
            eager = g.multilayer_sample_with_edge_attributes(seeds, [m, m], names, weight_name, random_seeds=hop_seeds)
            before = binding.lib().wholememory_ext_edge_chain_calls()
            pending = g.multilayer_sample_begin(seeds, [m, m], random_seeds=hop_seeds, weight_name=weight_name, edge_attr_names=names)
            assert binding.lib().wholememory_ext_edge_chain_calls() == before + 1, "not queued as one chain: " + what
            padded = pending.padded_frontier
            out = torch.full((padded.shape[0], dim), -7.0, device="cuda")
            emb.gather(padded, out=out)                      # queued behind the sampling kernels, before result()
            got = pending.result()
            torch.cuda.synchronize()
            assert len(got) == 5 and len(eager) == 5, what
            for k, (a_list, b_list) in enumerate(zip(got, eager)):
                assert len(a_list) == len(b_list), (what, k)
                for layer, (a, b) in enumerate(zip(a_list, b_list)):
                    pairs = [(a[name], b[name]) for name in names] if isinstance(a, dict) else [(a, b)]
                    for x, y in pairs:
                        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, k, layer)
            n = got[0][0].shape[0]
            assert padded.shape[0] > n, what                 # the chain handed out its upper-bound array
            assert torch.equal(padded[:n], got[0][0]) and bool((padded[n:] == -1).all()), what
            assert torch.equal(out[:n], emb.gather(got[0][0])) and bool((out[n:] == -7.0).all()), what
            assert torch.equal(out[:n, 0], got[0][0].float()), what      # (row v of the table starts with v)
    torch.cuda.synchronize()
    comm.barrier()
    wgth.destroy_embedding(emb)


# ------------------------------------------------------------------------------------------------ a DISTRIBUTED graph
def check_not_implemented(h, starts, ops):
    """the named ops have no DISTRIBUTED route and say WHOLEMEMORY_NOT_IMPLEMENTED"""
    import pytest
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd import binding
    dev_starts = _dev(starts)
    p, q = N2V_PQ
    calls = {"random_walk": lambda: wops.random_walk(h.row, h.col, dev_starts, STEPS, 1),
             "node2vec_walk": lambda: wops.node2vec_walk(h.row, h.col, dev_starts, STEPS, p, q, 1),
             "negative_sample": lambda: wops.negative_sample(h.row, h.col, dev_starts, NEGATIVES, 1),
             "induced_subgraph": lambda: wops.induced_subgraph(h.row, h.col, dev_starts)}
    for name in ops:
        with pytest.raises(binding.WholeMemoryError) as e:
            calls[name]()
        assert e.value.code == 2 and isinstance(e.value, NotImplementedError), name      # WHOLEMEMORY_NOT_IMPLEMENTED
