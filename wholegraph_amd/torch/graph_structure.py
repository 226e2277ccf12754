"""One relation of a graph held in WholeMemory as CSR arrays, and the samplers that walk it.

Public surface = ``pylibwholegraph.torch.graph_structure.GraphStructure`` (reference
``python/pylibwholegraph/pylibwholegraph/torch/graph_structure.py:21-228``: same method names, arguments and return
layouts, so cuGraph-DGL / PyG call sites keep working). The bodies are this package's own: the CSR pair is validated once
in a helper, attributes live in one registry keyed by kind, and the multi-hop sampler is a loop over a per-hop record
instead of four parallel lists. Extensions: ``multilayer_sample_without_replacement(..., random_seeds=[...])`` fixes the
per-hop sampler seeds (the reference draws them from the global RNG), which is what lets tests/test_c5_flow_gpu.py replay
the whole chain on the CPU oracle; a multi-hop sample (unweighted, or weighted by an edge attribute) on a CSR mapped into this
rank runs as ONE library call with ONE host round trip for all hops (``wholegraph_ops.multilayer_sample``: upper-bound-sized buffers, counts kept on the
device, views trimmed at the end; ``WM_MULTILAYER_CHAIN=0`` switches it off), and where that does not apply a hop still runs as
one call (``wholegraph_ops.sample_append_unique``: sampler + append_unique with a single host round trip, same outputs).
``multilayer_sample_with_edge_attributes`` and ``multilayer_sample_begin(..., edge_attr_names=[...])`` take the same two routes
with the graph edge id of every sample carried along, the attributes fetched on the device behind each hop.
"""
import os
import random
from collections import namedtuple
from typing import List, Optional, Sequence, Union

import torch

from .. import binding as wmb
from . import graph_ops, wholegraph_ops
from .tensor import WholeMemoryTensor

_INDEX_DTYPES = (torch.int32, torch.int64)
_Hop = namedtuple("_Hop", "targets edge_index row_ptr col_ind")


def _layer_lists(layers, node_ids):
    return ([hop.targets for hop in layers] + [node_ids], [hop.edge_index for hop in layers],
            [hop.row_ptr for hop in layers], [hop.col_ind for hop in layers])


def _chain_layers(chain, hops):
    layers = [None] * hops
    for depth, (offsets, widened, neighbour_pos, centre_lid, edge_index) in enumerate(chain):
        layers[hops - 1 - depth] = _Hop(widened, edge_index, offsets, neighbour_pos)
    return layers


class _DeferredSample(object):
    """handle of GraphStructure.multilayer_sample_begin; `edge_attrs` = (names, names fetched by the chain) when the sample
    carries edge attributes"""

    def __init__(self, graph, node_ids, max_neighbors, random_seeds, pending, weight_name=None, edge_attrs=None):
        self._node_ids, self._hops, self._pending, self._lists = node_ids, len(max_neighbors), pending, None
        self._graph, self._edge_attrs = graph, edge_attrs
        if pending is None:      # not queued as one chain: sampled now, hop by hop
            if edge_attrs is None:
                self._lists = graph._sample_hop_by_hop(node_ids, max_neighbors, weight_name, random_seeds)
            else:
                self._lists = graph._sample_hop_by_hop_with_edges(node_ids, max_neighbors, edge_attrs[0], weight_name, random_seeds)
            self.padded_frontier = self._lists[0][0]
        else:
            self.padded_frontier = pending.padded_frontier

    def result(self):
        if self._lists is None:
            chain = self._pending.finish()
            self._lists = _layer_lists(_chain_layers([hop[:5] for hop in chain], self._hops), self._node_ids)
            if self._edge_attrs is not None:
                self._lists += (self._graph._chain_edge_attrs(chain, *self._edge_attrs),)
        return self._lists


def _checked_csr(row_ptr: WholeMemoryTensor, col_ind: WholeMemoryTensor):
    """(node count, edge count) of a valid CSR pair; raises AssertionError like the reference on a malformed one"""
    problems = []
    if row_ptr.dim() != 1 or col_ind.dim() != 1:
        problems.append("csr_row_ptr and csr_col_ind must be 1-D")
    if row_ptr.dtype != torch.int64:
        problems.append("csr_row_ptr must be int64")
    if col_ind.dtype not in _INDEX_DTYPES:
        problems.append("csr_col_ind must be int32 or int64")
    if row_ptr.dim() == 1 and row_ptr.shape[0] < 2:
        problems.append("csr_row_ptr needs at least two entries")
    assert not problems, "; ".join(problems)
    return row_ptr.shape[0] - 1, col_ind.shape[0]


class GraphStructure(object):
    """CSR structure of one relation + per-node / per-edge attribute tensors (all WholeMemory tensors)."""

    def __init__(self):
        self.csr_row_ptr = self.csr_col_ind = None
        self.node_count = self.edge_count = 0
        self._attributes = {"node": {}, "edge": {}}

    # the reference exposes the two registries as plain dict attributes
    @property
    def node_attributes(self):
        return self._attributes["node"]

    @property
    def edge_attributes(self):
        return self._attributes["edge"]

    def set_csr_graph(self, csr_row_ptr: WholeMemoryTensor, csr_col_ind: WholeMemoryTensor):
        self.node_count, self.edge_count = _checked_csr(csr_row_ptr, csr_col_ind)
        self.csr_row_ptr, self.csr_col_ind = csr_row_ptr, csr_col_ind

    def _register(self, kind: str, name: str, tensor: WholeMemoryTensor, expected_rows: int):
        registry = self._attributes[kind]
        assert name not in registry, "%s attribute %r is already set" % (kind, name)
        assert tensor.shape[0] == expected_rows, "%s attribute %r has %d rows, the graph has %d %ss" % (
            kind, name, tensor.shape[0], expected_rows, kind)
        registry[name] = tensor

    def set_node_attribute(self, attr_name: str, attr_tensor: WholeMemoryTensor):
        self._register("node", attr_name, attr_tensor, self.node_count)

    def set_edge_attribute(self, attr_name: str, attr_tensor: WholeMemoryTensor):
        self._register("edge", attr_name, attr_tensor, self.edge_count)

    def _weights(self, weight_name: Optional[str]):
        """handle of the edge attribute a weighted sample draws by; None = unweighted"""
        if weight_name is None:
            return None
        assert weight_name in self.edge_attributes, "no edge attribute named %r" % weight_name
        return self.edge_attributes[weight_name].wmb_tensor

    # ------------------------------------------------------------------------------------------- one hop
    def _one_hop(self, centers: torch.Tensor, fanout: int, weight_name: Optional[str], seed, want_lid: bool, want_eid: bool):
        csr = (self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor)
        if weight_name is None:
            return wholegraph_ops.unweighted_sample_without_replacement(*csr, centers, fanout, seed, want_lid, want_eid)
        return wholegraph_ops.weighted_sample_without_replacement(*csr, self._weights(weight_name), centers, fanout, seed,
                                                                  want_lid, want_eid)

    def unweighted_sample_without_replacement_one_hop(self, center_nodes_tensor: torch.Tensor, max_sample_count: int, *,
                                                      random_seed: Union[int, None] = None,
                                                      need_center_local_output: bool = False,
                                                      need_edge_output: bool = False):
        """-> csr_row_ptr, sampled_nodes[, center_node_local_id][, edge_index]"""
        return self._one_hop(center_nodes_tensor, max_sample_count, None, random_seed, need_center_local_output,
                             need_edge_output)

    def weighted_sample_without_replacement_one_hop(self, weight_name: str, center_nodes_tensor: torch.Tensor,
                                                    max_sample_count: int, *, random_seed: Union[int, None] = None,
                                                    need_center_local_output: bool = False,
                                                    need_edge_output: bool = False):
        """the same, neighbours drawn with probability proportional to the named edge attribute"""
        return self._one_hop(center_nodes_tensor, max_sample_count, weight_name, random_seed, need_center_local_output,
                             need_edge_output)

    # ------------------------------------------------------------------------------------------ random walks
    def random_walk(self, start_nodes: torch.Tensor, walk_length: int, *, weight_name: Optional[str] = None,
                    random_seed: Union[int, None] = None, need_edge_ids: bool = False):
        """Extension: one random walk of walk_length steps from every start node, all of them in one launch
        (``wholegraph_ops.random_walk``). -> walks [n, walk_length + 1][, edge_ids int64 [n, walk_length]]; -1 from the step at
        which a walk ends. weight_name: steps are drawn with probability proportional to the named edge attribute."""
        return wholegraph_ops.random_walk(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, start_nodes, walk_length,
                                          random_seed, wm_csr_weight_ptr_tensor=self._weights(weight_name),
                                          need_edge_output=need_edge_ids)

    def node2vec_walk(self, start_nodes: torch.Tensor, walk_length: int, p: float, q: float, *,
                      weight_name: Optional[str] = None, random_seed: Union[int, None] = None, col_sorted: bool = False,
                      need_edge_ids: bool = False):
        """Extension: one node2vec (p, q) walk of walk_length steps from every start node, all of them in one launch
        (``wholegraph_ops.node2vec_walk``). -> walks [n, walk_length + 1][, edge_ids int64 [n, walk_length]]; -1 from the step
        at which a walk ends. weight_name: the named edge attribute weighs the edges (else every edge weighs 1). col_sorted:
        the caller's promise that every row of csr_col_ind is ascending."""
        return wholegraph_ops.node2vec_walk(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, start_nodes, walk_length,
                                            p, q, random_seed, wm_csr_weight_ptr_tensor=self._weights(weight_name),
                                            col_sorted=col_sorted, need_edge_output=need_edge_ids)

    def negative_sample(self, src_nodes: torch.Tensor, num_negatives: int, *, mode: str = "uniform", exclude_edges: bool = True,
                        exclude_self: bool = True, max_tries: int = 8, random_seed: Union[int, None] = None,
                        col_sorted: bool = False):
        """Extension: num_negatives nodes per source node that are not its neighbours (exclude_edges) and not the node itself
        (exclude_self), all of them in one launch (``wholegraph_ops.negative_sample``). -> [n, num_negatives] in csr_col_ind's
        dtype; -1 where max_tries draws were all rejected or the source is not a node. mode: "uniform" over the nodes or
        "degree", by how often a node occurs in csr_col_ind. col_sorted: the caller's promise that every row of csr_col_ind
        is ascending."""
        return wholegraph_ops.negative_sample(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, src_nodes, num_negatives,
                                              random_seed, mode=mode, exclude_edges=exclude_edges, exclude_self=exclude_self,
                                              max_tries=max_tries, col_sorted=col_sorted)

    # ------------------------------------------------------------------------------------------ subgraphs
    def induced_subgraph(self, nodes: torch.Tensor, *, need_edge_output: bool = False,
                         edge_attr_names: Optional[Sequence[str]] = None):
        """Extension: every graph edge among `nodes` as one local CSR block (``wholegraph_ops.induced_subgraph``), the batch
        of subgraph-wise training. -> offsets int32 [n + 1], col int32 [m][, edge ids int64 [m]][, {name: attribute of the kept
        edges}]. Row i belongs to nodes[i]; col holds positions in `nodes`. edge_attr_names: the named edge attributes (or
        "__edge_id__") at the kept edges, aligned with col."""
        names = None if edge_attr_names is None else self._checked_edge_attr_names(edge_attr_names)
        out = wholegraph_ops.induced_subgraph(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, nodes,
                                              need_edge_output=need_edge_output or names is not None)
        if names is None:
            return out
        offsets, col, edge_id = out
        attrs = self._edge_attr_dict(names, edge_id)
        return (offsets, col, edge_id, attrs) if need_edge_output else (offsets, col, attrs)

    def saint_random_walk_subgraph(self, roots: torch.Tensor, walk_length: int, *, random_seed: Union[int, None] = None,
                                   weight_name: Optional[str] = None, need_edge_output: bool = False):
        """Extension: the GraphSAINT random-walk sampler. One walk of walk_length steps from every root (``random_walk``), the
        distinct nodes the walks visit in ascending order, and the subgraph they induce (``induced_subgraph``).
        -> nodes, offsets int32 [n + 1], col int32 [m][, edge ids int64 [m]]. The node order, and with it the whole result,
        depends on the roots and the seed alone. The loss-normalisation coefficients of GraphSAINT are not computed here."""
        walks = self.random_walk(roots, walk_length, weight_name=weight_name, random_seed=random_seed)
        nodes = torch.unique(walks[walks >= 0])     # (sorted)
        return (nodes,) + tuple(self.induced_subgraph(nodes, need_edge_output=need_edge_output))

    # ------------------------------------------------------------------------------------------ temporal sampling
    def _edge_times(self, time_name: str):
        assert time_name in self.edge_attributes, "no edge attribute named %r" % time_name
        times = self.edge_attributes[time_name]
        assert times.dim() == 1 and times.dtype == torch.int64, "edge attribute %r must be 1-D int64 timestamps" % time_name
        return times

    def temporal_sample_one_hop(self, time_name: str, center_nodes_tensor: torch.Tensor, center_times_tensor: torch.Tensor,
                                max_sample_count: int, *, strategy: str = "uniform", inclusive: bool = True,
                                time_window: Union[int, None] = None, random_seed: Union[int, None] = None,
                                need_center_local_output: bool = False, need_edge_output: bool = False):
        """Extension: for centre i, the node center_nodes_tensor[i] at the time center_times_tensor[i], up to max_sample_count
        neighbours whose edge is not in that time's future (``wholegraph_ops.temporal_sample_without_replacement``);
        `time_name` names the int64 edge attribute that holds the edge times.
        -> csr_row_ptr, sampled_nodes[, center_node_local_id][, edge_index]"""
        return wholegraph_ops.temporal_sample_without_replacement(
            self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, self._edge_times(time_name).wmb_tensor, center_nodes_tensor,
            center_times_tensor, max_sample_count, random_seed, need_center_local_output, need_edge_output, strategy=strategy,
            inclusive=inclusive, time_window=time_window)

    def multilayer_temporal_sample(self, node_ids: torch.Tensor, node_times: torch.Tensor, max_neighbors: List[int],
                                   time_name: str, *, strategy: str = "uniform", inclusive: bool = True,
                                   time_window: Union[int, None] = None, propagate: str = "seed",
                                   random_seeds: Optional[Sequence[int]] = None,
                                   edge_attr_names: Optional[Sequence[str]] = None):
        """Extension: len(max_neighbors) temporal hops outwards from the (node, time) seeds, sampled as DISJOINT TREES, which
        is what temporal sampling requires (PyG's NeighborLoader with time_attr): the same node reached under two different
        times is two computational nodes, so nothing is de-duplicated. Hop h has the centres C_h at the times T_h, C_0 =
        node_ids; C_{h+1} = cat(C_h, neighbours_h) and T_{h+1} = cat(T_h, inherited), where a neighbour inherits the time of
        its centre (propagate="seed", the PyG rule) or the time of the edge that led to it ("edge", the TGAT rule: a deeper
        edge is never later than the edge above it). The block of hop h is csr_row_ptr = the sampler's offsets and csr_col_ind
        = len(C_h) + arange(E_h) in int32. Returns lists indexed by layer, OUTERMOST layer first, as
        multilayer_sample_without_replacement does: target_gids and target_times (hops + 1 entries, the last ones node_ids and
        node_times), edge_indice [2, E_h] (row 0 the position of the neighbour, row 1 of its centre, in target_gids[i]),
        csr_row_ptr, csr_col_ind, edge_ids (int64 positions in the graph's csr_col_ind) and, with edge_attr_names, the
        attribute dicts of multilayer_sample_with_edge_attributes."""
        if propagate not in ("seed", "edge"):
            raise ValueError("propagate must be 'seed' or 'edge', got %r" % (propagate,))
        hops = len(max_neighbors)
        if random_seeds is not None:
            assert len(random_seeds) == hops, "one seed per hop"
        names = None if edge_attr_names is None else self._checked_edge_attr_names(edge_attr_names)
        times = self._edge_times(time_name)
        gids, gtimes = [node_ids], [node_times]
        edge_indice, row_ptrs, col_inds, edge_ids, attrs = [], [], [], [], []
        for depth, fanout in enumerate(max_neighbors):          # depth 0 = next to the seeds = layer hops - 1
            centres, centre_times = gids[0], gtimes[0]
            offsets, neighbours, centre_lid, edge_id = self.temporal_sample_one_hop(
                time_name, centres, centre_times, fanout, strategy=strategy, inclusive=inclusive, time_window=time_window,
                random_seed=None if random_seeds is None else random_seeds[depth], need_center_local_output=True,
                need_edge_output=True)
            inherited = centre_times[centre_lid.long()] if propagate == "seed" else times.gather(edge_id)
            col = centres.shape[0] + torch.arange(neighbours.shape[0], device=neighbours.device, dtype=torch.int32)
            gids.insert(0, torch.cat([centres, neighbours.to(centres.dtype)]))
            gtimes.insert(0, torch.cat([centre_times, inherited]))
            edge_indice.insert(0, torch.stack([col, centre_lid]))
            row_ptrs.insert(0, offsets)
            col_inds.insert(0, col)
            edge_ids.insert(0, edge_id)
            if names is not None:
                attrs.insert(0, self._edge_attr_dict(names, edge_id))
        out = (gids, gtimes, edge_indice, row_ptrs, col_inds, edge_ids)
        return out if names is None else out + (attrs,)

    # ------------------------------------------------------------------------------------------ several hops
    def multilayer_sample_without_replacement(self, node_ids: torch.Tensor, max_neighbors: List[int],
                                              weight_name: Union[str, None] = None, *,
                                              random_seeds: Optional[Sequence[int]] = None):
        """Sample len(max_neighbors) hops outwards from node_ids (max_neighbors[0] is the fan-out of the hop next to the
        seeds). Returns four lists indexed by layer, OUTERMOST layer first, as the reference does:
          target_gids  (hops + 1 entries; the last one is node_ids, entry i holds entry i + 1 followed by its new neighbours)
          edge_indice  [2, n_edges]: row 0 = position of the neighbour in target_gids[i], row 1 = position of its centre
          csr_row_ptr / csr_col_ind of the sampled block (col_ind = row 0 of edge_indice)"""
        hops = len(max_neighbors)
        if random_seeds is not None:
            assert len(random_seeds) == hops, "one seed per hop"
        if hops > 0 and os.environ.get("WM_MULTILAYER_CHAIN", "1") != "0":
            # the whole chain as one library call with a single host round trip (extension); None = not applicable to this
            # graph or these sizes: hop by hop below then
            chain = wholegraph_ops.multilayer_sample(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, node_ids,
                                                     max_neighbors, random_seeds,
                                                     wm_csr_weight_ptr_tensor=self._weights(weight_name))
            if chain is not None:
                return _layer_lists(_chain_layers(chain, hops), node_ids)
        return self._sample_hop_by_hop(node_ids, max_neighbors, weight_name, random_seeds)

    def multilayer_sample_begin(self, node_ids: torch.Tensor, max_neighbors: List[int], *,
                                random_seeds: Optional[Sequence[int]] = None, weight_name: Optional[str] = None,
                                edge_attr_names: Optional[Sequence[str]] = None):
        """Extension: the multi-layer sample (weighted by the edge attribute `weight_name` when given) QUEUED, the host not
        waiting for it. Returns a handle with
          .padded_frontier   the outermost frontier (what target_gids[0] will be) at its upper-bound size, the entries behind the
                             sampled nodes set to -1 — hand it to WholeMemoryEmbedding.gather right away: negative ids are
                             skipped, so rows [0, n) of that gather's output are the features of target_gids[0];
          .result()          one stream synchronise, then exactly what multilayer_sample_without_replacement returns.
        The feature gather of a mini-batch then runs back to back with the sampling kernels instead of behind a host round
        trip. When the one-call chain does not apply (see wholegraph_ops.multilayer_sample_begin) the sample is taken here and
        now, hop by hop, and padded_frontier is target_gids[0] itself.
        edge_attr_names (keyword): .result() returns the five lists of multilayer_sample_with_edge_attributes for these
        names; the attributes are fetched on the device behind each hop, still without the host waiting."""
        hops = len(max_neighbors)
        if random_seeds is not None:
            assert len(random_seeds) == hops, "one seed per hop"
        if edge_attr_names is not None:
            names = self._checked_edge_attr_names(edge_attr_names)
            if random_seeds is None:
                random_seeds = [random.getrandbits(64) for _ in range(hops)]
            pending, fetched = self._edge_chain_begin(node_ids, max_neighbors, names, weight_name, random_seeds)
            return _DeferredSample(self, node_ids, max_neighbors, random_seeds, pending, weight_name, (names, fetched))
        pending = None
        if hops > 0 and os.environ.get("WM_MULTILAYER_CHAIN", "1") != "0":
            pending = wholegraph_ops.multilayer_sample_begin(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, node_ids,
                                                             max_neighbors, random_seeds,
                                                             wm_csr_weight_ptr_tensor=self._weights(weight_name))
        return _DeferredSample(self, node_ids, max_neighbors, random_seeds, pending, weight_name)

    # ------------------------------------------------------------------------------- several hops, with edge attributes
    def _checked_edge_attr_names(self, edge_attr_names):
        names = list(edge_attr_names)
        for name in names:
            assert name == "__edge_id__" or name in self.edge_attributes, "no edge attribute named %r" % name
        return names

    def _chain_takes_edge_attribute(self, tensor: WholeMemoryTensor):
        """what the chain's attribute kernel fetches (wholememory_ext_multilayer_sample_edges): 1-D, 4- or 8-byte elements,
        mapped into this rank; anything else is gathered by edge id afterwards"""
        if tensor.dim() != 1 or torch.tensor([], dtype=tensor.dtype).element_size() not in (4, 8):
            return False
        return wmb.lib().wholememory_get_memory_type(tensor._handle()) in (wmb.MT_CONTINUOUS, wmb.MT_CHUNKED)

    def _edge_chain_begin(self, node_ids, max_neighbors, names, weight_name, random_seeds):
        """(the chain with edge ids queued or None, names of the attributes it fetches)"""
        if len(max_neighbors) == 0 or os.environ.get("WM_MULTILAYER_CHAIN", "1") == "0":
            return None, []
        fetched = []
        for name in names:
            if name != "__edge_id__" and name not in fetched and self._chain_takes_edge_attribute(self.edge_attributes[name]):
                fetched.append(name)
        pending = wholegraph_ops.multilayer_sample_begin(
            self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, node_ids, max_neighbors, random_seeds,
            wm_csr_weight_ptr_tensor=self._weights(weight_name), need_edge_ids=True,
            wm_edge_attr_tensors=[self.edge_attributes[name] for name in fetched] if fetched else None)
        return pending, fetched

    def _edge_attr_dict(self, names, edge_id, fetched=None):
        fetched = fetched or {}
        return {name: edge_id if name == "__edge_id__" else fetched[name] if name in fetched
                else self.edge_attributes[name].gather(edge_id) for name in names}

    def _chain_edge_attrs(self, chain, names, fetched_names):
        """the fifth list (outermost layer first) from the per-hop tuples of the chain with edge ids"""
        hops = len(chain)
        attrs = [None] * hops
        for depth, hop in enumerate(chain):
            fetched = dict(zip(fetched_names, hop[6])) if fetched_names else None
            attrs[hops - 1 - depth] = self._edge_attr_dict(names, hop[5], fetched)
        return attrs

    def _sample_hop_by_hop_with_edges(self, node_ids, max_neighbors, names, weight_name, random_seeds):
        hops = len(max_neighbors)
        layers, attrs = [None] * hops, [None] * hops
        frontier = node_ids
        for depth, fanout in enumerate(max_neighbors):          # depth 0 = next to the seeds = layer hops - 1
            seed = None if random_seeds is None else random_seeds[depth]
            # the fused hop with edge ids (one host round trip); None = not applicable to this graph: the two ops then
            fused = wholegraph_ops.sample_append_unique(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, frontier,
                                                        fanout, seed, wm_csr_weight_ptr_tensor=self._weights(weight_name),
                                                        need_edge_output=True)
            if fused is not None:
                offsets, widened, neighbour_pos, centre_lid, edge_id = fused
            else:
                offsets, neighbours, centre_lid, edge_id = self._one_hop(frontier, fanout, weight_name, seed, True, True)
                widened, neighbour_pos = graph_ops.append_unique(frontier, neighbours, need_neighbor_raw_to_unique=True)
            layers[hops - 1 - depth] = _Hop(widened, torch.stack([neighbour_pos, centre_lid]), offsets, neighbour_pos)
            attrs[hops - 1 - depth] = self._edge_attr_dict(names, edge_id)
            frontier = widened
        return _layer_lists(layers, node_ids) + (attrs,)

    def multilayer_sample_with_edge_attributes(self, node_ids: torch.Tensor, max_neighbors: List[int],
                                               edge_attr_names: Sequence[str], weight_name: Union[str, None] = None, *,
                                               random_seeds: Optional[Sequence[int]] = None):
        """Extension: multilayer_sample_without_replacement plus the attributes of the SAMPLED edges. Returns its four lists
        and a fifth, per layer (outermost first) a dict {name: tensor [n_edges]} aligned with that layer's csr_col_ind:
        entry e is the named edge attribute at the graph edge that block edge e was drawn from. The name "__edge_id__"
        delivers those int64 graph edge ids (positions in the graph's csr_col_ind) themselves. Routes, first that applies:
        the one-call chain with edge ids (``wholegraph_ops.multilayer_sample(..., need_edge_ids=True)``: one host round trip
        for all hops, 1-D attributes of 4- or 8-byte elements mapped into this rank fetched on the device behind each hop;
        ``WM_MULTILAYER_CHAIN=0`` switches it off), the fused hop with edge ids hop by hop, the one-hop sampler with edge
        output + append_unique. Attributes the chain does not fetch are gathered by edge id afterwards. Every route returns
        the same values; with the same random_seeds the four lists equal multilayer_sample_without_replacement's. Without
        random_seeds one 64-bit seed per hop is drawn from `random`, in hop order."""
        names = self._checked_edge_attr_names(edge_attr_names)
        hops = len(max_neighbors)
        if random_seeds is not None:
            assert len(random_seeds) == hops, "one seed per hop"
        else:
            random_seeds = [random.getrandbits(64) for _ in range(hops)]
        pending, fetched = self._edge_chain_begin(node_ids, max_neighbors, names, weight_name, random_seeds)
        if pending is not None:
            chain = pending.finish()
            return _layer_lists(_chain_layers([hop[:5] for hop in chain], hops), node_ids) + (
                self._chain_edge_attrs(chain, names, fetched),)
        return self._sample_hop_by_hop_with_edges(node_ids, max_neighbors, names, weight_name, random_seeds)

    def _sample_hop_by_hop(self, node_ids, max_neighbors, weight_name, random_seeds):
        hops = len(max_neighbors)
        layers = [None] * hops
        frontier = node_ids
        for depth, fanout in enumerate(max_neighbors):          # depth 0 = next to the seeds = layer hops - 1
            seed = None if random_seeds is None else random_seeds[depth]
            # sampler + append_unique as one library call with one host round trip (extension); None = not applicable
            # to this graph (CSR not mapped into this rank, id dtypes differ ...): the two ops below then
            fused = wholegraph_ops.sample_append_unique(self.csr_row_ptr.wmb_tensor, self.csr_col_ind.wmb_tensor, frontier,
                                                        fanout, seed, wm_csr_weight_ptr_tensor=self._weights(weight_name))
            if fused is not None:
                offsets, widened, neighbour_pos, centre_lid = fused
            else:
                offsets, neighbours, centre_lid = self._one_hop(frontier, fanout, weight_name, seed, True, False)
                widened, neighbour_pos = graph_ops.append_unique(frontier, neighbours, need_neighbor_raw_to_unique=True)
            layers[hops - 1 - depth] = _Hop(widened, torch.stack([neighbour_pos, centre_lid]), offsets, neighbour_pos)
            frontier = widened
        return _layer_lists(layers, node_ids)
