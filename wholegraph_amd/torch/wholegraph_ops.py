"""Neighbour sampling on CSR graphs stored in WholeMemory.

Mirror of ``python/pylibwholegraph/pylibwholegraph/torch/wholegraph_ops.py:27-209`` over the C ABI of
``include/wholememory/wholegraph_op.h``. `wm_csr_*_tensor` arguments are `wholememory_tensor_t` handles
(``WholeMemoryTensor.wmb_tensor``), exactly what the reference functions take."""
import ctypes as C
import math
import random
from typing import Union

import torch

from .. import binding as wmb
from .utils import wholememory_dtype_to_torch_dtype
from .wholegraph_env import TorchMemoryContext, get_stream, get_wholegraph_env_fns, op_device, wrap_torch_tensor


def _handle(t):
    return t.wmb_tensor if hasattr(t, "wmb_tensor") else t


def _tensor_dim(h):
    return int(wmb.lib().wholememory_tensor_get_tensor_description(h).contents.dim)


def _seed64(random_seed):
    """the seed as the C ABI takes it; 64 random bits when the caller gave none"""
    if random_seed is None:
        random_seed = random.getrandbits(64)
    return C.c_ulonglong(int(random_seed) & 0xFFFFFFFFFFFFFFFF)


def _col_dtype(col_handle):
    """the torch dtype of csr_col_ptr, which is that of every output that holds node ids"""
    return wholememory_dtype_to_torch_dtype(wmb.lib().wholememory_tensor_get_tensor_description(col_handle).contents.dtype)


def _sample_outputs(offset, dest, lid, egid, need_center_local_output, need_edge_output):
    if need_edge_output and need_center_local_output:
        return offset, dest.get_tensor(), lid.get_tensor(), egid.get_tensor()
    if need_center_local_output:
        return offset, dest.get_tensor(), lid.get_tensor()
    if need_edge_output:
        return offset, dest.get_tensor(), egid.get_tensor()
    return offset, dest.get_tensor()


def unweighted_sample_without_replacement(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, center_nodes_tensor: torch.Tensor,
                                          max_sample_count: int, random_seed: Union[int, None] = None,
                                          need_center_local_output: bool = False, need_edge_output: bool = False):
    """For every center node, min(degree, max_sample_count) distinct neighbours (all when max_sample_count <= 0).
    Returns (sample_offset int32 [n + 1], sampled node ids[, center local id int32][, edge id int64])."""
    row, col = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor)
    assert _tensor_dim(row) == 1
    assert _tensor_dim(col) == 1
    assert center_nodes_tensor.dim() == 1
    offset = torch.empty(center_nodes_tensor.shape[0] + 1, device=op_device(), dtype=torch.int)
    dest = TorchMemoryContext()
    lid = TorchMemoryContext() if need_center_local_output else None
    egid = TorchMemoryContext() if need_edge_output else None
    wc, wo = wrap_torch_tensor(center_nodes_tensor), wrap_torch_tensor(offset)
    wmb.check(wmb.lib().wholegraph_csr_unweighted_sample_without_replacement(
        row, col, wc.handle, int(max_sample_count), wo.handle, C.c_void_p(dest.get_c_context()),
        C.c_void_p(lid.get_c_context() if lid else 0), C.c_void_p(egid.get_c_context() if egid else 0),
        _seed64(random_seed), get_wholegraph_env_fns(), C.c_void_p(get_stream())))
    return _sample_outputs(offset, dest, lid, egid, need_center_local_output, need_edge_output)


def sample_append_unique(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, center_nodes_tensor: torch.Tensor, max_sample_count: int,
                         random_seed: Union[int, None] = None, *, wm_csr_weight_ptr_tensor=None, need_edge_output: bool = False):
    """Extension (include/wholememory/wholegraph_amd_ext.h): one hop = unweighted sampling + append_unique(center nodes,
    sampled neighbours) in ONE call with one host round trip. Returns (sample_offset int32 [n + 1], unique nodes, position of
    every sampled neighbour in `unique` int32, center local id int32) — or None when the library declines (CSR not mapped
    into this rank, dtypes differ, empty frontier, max_sample_count <= 0): run the two ops then.
    wm_csr_weight_ptr_tensor (keyword): the hop samples with the weighted sampler on these edge weights; also declined for a
    weight tensor that is not mapped, not float / double or not one entry per edge, and for max_sample_count > 8192.
    need_edge_output (keyword): a fifth tensor, the int64 graph edge id (position in csr_col_ptr) of every sampled neighbour
    (wholememory_ext_sample_append_unique_edges); declined in the same cases."""
    row, col = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor)
    assert center_nodes_tensor.dim() == 1
    offset = torch.empty(center_nodes_tensor.shape[0] + 1, device=op_device(), dtype=torch.int)
    uniq, pos, lid = TorchMemoryContext(), TorchMemoryContext(), TorchMemoryContext()
    wc, wo = wrap_torch_tensor(center_nodes_tensor), wrap_torch_tensor(offset)
    tail = (int(max_sample_count), _seed64(random_seed), wo.handle, C.c_void_p(uniq.get_c_context()),
            C.c_void_p(pos.get_c_context()), C.c_void_p(lid.get_c_context()), get_wholegraph_env_fns(), C.c_void_p(get_stream()))
    egid = TorchMemoryContext() if need_edge_output else None
    if need_edge_output:
        wgt = None if wm_csr_weight_ptr_tensor is None else _handle(wm_csr_weight_ptr_tensor)
        rc = wmb.lib().wholememory_ext_sample_append_unique_edges(row, col, wgt, wc.handle, *tail[:6],
                                                                  C.c_void_p(egid.get_c_context()), *tail[6:])
    elif wm_csr_weight_ptr_tensor is None:
        rc = wmb.lib().wholememory_ext_sample_append_unique(row, col, wc.handle, *tail)
    else:
        rc = wmb.lib().wholememory_ext_weighted_sample_append_unique(row, col, _handle(wm_csr_weight_ptr_tensor), wc.handle, *tail)
    if rc == wmb.NOT_SUPPORTED:
        return None
    wmb.check(rc)
    if need_edge_output:
        return offset, uniq.get_tensor(), pos.get_tensor(), lid.get_tensor(), egid.get_tensor()
    return offset, uniq.get_tensor(), pos.get_tensor(), lid.get_tensor()


_pinned_pool = {}     # hops -> idle pinned count buffers (one per chain in flight, handed back by finish())
_event_pool = []


def _multilayer_budget_bytes():
    """upper-bound buffers of a chain that the one-call route may allocate (WM_MULTILAYER_MAX_BYTES, default 8 GiB): beyond it
    the chain is declined and the caller samples hop by hop with exactly sized outputs"""
    import os
    try:
        return int(os.environ.get("WM_MULTILAYER_MAX_BYTES", str(8 << 30)))
    except ValueError:
        return 8 << 30


def _compact(t):
    """a trimmed view keeps its whole upper-bound buffer alive: copy out of big, mostly empty ones"""
    room = t.untyped_storage().nbytes()
    return t.clone() if room > (16 << 20) and t.numel() * t.element_size() * 2 < room else t


class PendingMultilayerSample:
    """A multi-hop sample whose kernels are queued and whose counts the host has not read yet (multilayer_sample_begin).
    `padded_frontier` is the outermost frontier at its full upper-bound size, the entries behind the sampled nodes set to -1:
    it can be handed to a gather right away (negative ids are skipped). `finish()` synchronises the stream once, trims every
    output and returns what multilayer_sample returns. `edge_ids` / `edge_attrs` (per hop: the int64 edge ids and a list of
    attribute tensors, at their upper-bound sizes) add a sixth / seventh entry to every hop's tuple."""

    def __init__(self, hops, n0, offsets, uniques, edges, counts, stream, edge_ids=None, edge_attrs=None):
        self._hops, self._n0, self._offsets, self._uniques, self._edges = hops, n0, offsets, uniques, edges
        self._edge_ids, self._edge_attrs = edge_ids, edge_attrs
        self._counts, self._result = counts, None
        self.padded_frontier = uniques[-1]
        # finish() waits for THIS chain, not for whatever the caller queues behind it (the feature gather on padded_frontier
        # keeps running while the host trims the outputs)
        # (a chain queued while the stream is being captured into a graph has no event of its own: after the replay the
        # caller's stream is waited for instead)
        self._stream, self._done = stream, None
        if not torch.cuda.is_current_stream_capturing():
            self._done = _event_pool.pop() if _event_pool else torch.cuda.Event()
            self._done.record(stream)

    def finish(self):
        if self._result is not None:
            return self._result
        if self._done is not None:
            self._done.synchronize()      # the one host round trip of the whole chain
            _event_pool.append(self._done)
            self._done = None
        else:
            self._stream.synchronize()
        got = self._counts.tolist()
        _pinned_pool.setdefault(self._hops, []).append(self._counts)
        self._counts = None
        out, n_c = [], self._n0
        for h in range(self._hops):
            n_samples, n_new = got[2 * h], got[2 * h + 1]
            edge = _compact(self._edges[h][:, :n_samples])
            # (the outermost frontier stays a view of the padded array a gather may still be reading)
            uniq = self._uniques[h][:n_c + n_new] if h == self._hops - 1 else _compact(self._uniques[h][:n_c + n_new])
            hop = (_compact(self._offsets[h][:n_c + 1]), uniq, edge[0], edge[1], edge)
            if self._edge_ids is not None:
                hop += (_compact(self._edge_ids[h][:n_samples]),)
            if self._edge_attrs is not None:
                hop += ([_compact(t[:n_samples]) for t in self._edge_attrs[h]],)
            out.append(hop)
            n_c += n_new
        self.n_frontier = n_c
        self._result = out
        return out


def multilayer_sample_begin(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, seed_nodes_tensor: torch.Tensor, max_sample_counts,
                            random_seeds=None, *, wm_csr_weight_ptr_tensor=None, need_edge_ids: bool = False,
                            wm_edge_attr_tensors=None):
    """Queues every hop of an unweighted multi-layer sample (wholememory_ext_multilayer_sample: one library call, counts kept
    on the device between hops, no host round trip) and returns a PendingMultilayerSample WITHOUT waiting — or None when the
    library declines (CSR not mapped into this rank, dtypes differ, empty seeds, upper bounds beyond append_unique's hash-table
    route or beyond the memory budget, allocation failure): run hop by hop then.
    wm_csr_weight_ptr_tensor (keyword): every hop samples with the weighted sampler on these edge weights
    (wholememory_ext_multilayer_sample_weighted); also declined for a weight tensor that is not mapped, not float / double or
    not one entry per edge, and for a fan-out above 8192.
    need_edge_ids (keyword): every hop also delivers the int64 graph edge id of each sample
    (wholememory_ext_multilayer_sample_edges). wm_edge_attr_tensors (keyword, implies need_edge_ids): a sequence of edge
    attribute tensors whose values at the sampled edges are fetched on the device behind each hop, in the given order; the
    chain is also declined when one of them is not 1-D, not of 4- or 8-byte elements, not one entry per edge or not mapped
    into this rank."""
    row, col = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor)
    attr_handles = None if wm_edge_attr_tensors is None else [_handle(t) for t in wm_edge_attr_tensors]
    with_edges = bool(need_edge_ids) or attr_handles is not None
    n_attrs = 0 if attr_handles is None else len(attr_handles)
    if with_edges:
        wgt = None if wm_csr_weight_ptr_tensor is None else _handle(wm_csr_weight_ptr_tensor)
        attr_arr = (C.c_void_p * n_attrs)(*[getattr(h, "value", h) for h in attr_handles]) if n_attrs else None
        # (the edge id / attribute pointer arrays sit between center_lid and counts_host)
        chain = lambda *rest: wmb.lib().wholememory_ext_multilayer_sample_edges(
            row, col, wgt, *rest[:8], rest[11], n_attrs, attr_arr, rest[12], *rest[8:11])
    elif wm_csr_weight_ptr_tensor is None:
        chain = lambda *rest: wmb.lib().wholememory_ext_multilayer_sample(row, col, *rest[:11])
    else:
        wgt = _handle(wm_csr_weight_ptr_tensor)
        chain = lambda *rest: wmb.lib().wholememory_ext_multilayer_sample_weighted(row, col, wgt, *rest[:11])
    assert seed_nodes_tensor.dim() == 1
    hops = len(max_sample_counts)
    n0 = seed_nodes_tensor.shape[0]
    if hops == 0 or n0 == 0 or any(int(m) <= 0 for m in max_sample_counts):
        return None
    if random_seeds is None:
        random_seeds = [random.getrandbits(64) for _ in range(hops)]
    cap_c, cap_s = [n0], []
    for m in max_sample_counts:
        cap_s.append(cap_c[-1] * int(m))
        cap_c.append(cap_c[-1] + cap_s[-1])
    if cap_c[-1] >= (1 << 31) - 1:
        return None
    idt = seed_nodes_tensor.dtype
    # outputs + the library's scratch (ids, hash table of 2 slots per key, positions ...): ~ 10 words per sampled neighbour
    need = sum(4 * (cap_c[h] + 1) + idt.itemsize * cap_c[h + 1] + 8 * cap_s[h] + 40 * (cap_c[h] + cap_s[h]) for h in range(hops))
    attr_dtypes = []
    if with_edges:
        for h in attr_handles or ():
            attr_dtypes.append(wholememory_dtype_to_torch_dtype(
                wmb.lib().wholememory_tensor_get_tensor_description(h).contents.dtype))
        need += sum((8 + sum(dt.itemsize for dt in attr_dtypes)) * cap_s[h] for h in range(hops))
    if need > _multilayer_budget_bytes():
        return None
    fan = (C.c_int * hops)(*[int(m) for m in max_sample_counts])
    ws = wrap_torch_tensor(seed_nodes_tensor)
    # ask first (no buffers yet); anything but SUCCESS is a decline
    if chain(ws.handle, hops, fan, None, None, None, None, None, None, None, None, None, None) != wmb.WHOLEMEMORY_SUCCESS:
        return None
    dev = op_device()
    try:
        offsets = [torch.empty(cap_c[h] + 1, device=dev, dtype=torch.int) for h in range(hops)]
        uniques = [torch.empty(cap_c[h + 1], device=dev, dtype=idt) for h in range(hops)]
        edges = [torch.empty((2, max(cap_s[h], 1)), device=dev, dtype=torch.int) for h in range(hops)]   # row 0 positions, row 1 centre ids
        edge_ids = [torch.empty(max(cap_s[h], 1), device=dev, dtype=torch.int64) for h in range(hops)] if with_edges else None
        edge_attrs = None if attr_handles is None else [
            [torch.empty(max(cap_s[h], 1), device=dev, dtype=dt) for dt in attr_dtypes] for h in range(hops)]
    except torch.OutOfMemoryError:
        return None
    pool = _pinned_pool.setdefault(hops, [])
    counts = pool.pop() if pool else torch.zeros(2 * hops, dtype=torch.int32).pin_memory()
    rng = (C.c_ulonglong * hops)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in random_seeds])
    ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    egid_ptrs = ptrs(edge_ids) if with_edges else None
    attr_ptrs = ptrs([t for per_hop in edge_attrs for t in per_hop]) if n_attrs else None    # [h * n_attrs + k]
    try:
        rc = chain(ws.handle, hops, fan, rng, ptrs(offsets), ptrs(uniques), ptrs([e[0] for e in edges]),
                   ptrs([e[1] for e in edges]), C.c_void_p(counts.data_ptr()), get_wholegraph_env_fns(), C.c_void_p(get_stream()),
                   egid_ptrs, attr_ptrs)
    except torch.OutOfMemoryError:      # the library's scratch comes from torch's allocator through the env functions
        rc = wmb.NOT_SUPPORTED
    if rc != wmb.WHOLEMEMORY_SUCCESS:
        pool.append(counts)
        if rc in (wmb.NOT_SUPPORTED, wmb.OUT_OF_MEMORY):
            return None
        wmb.check(rc)
    return PendingMultilayerSample(hops, n0, offsets, uniques, edges, counts, torch.cuda.current_stream(), edge_ids, edge_attrs)


def multilayer_sample(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, seed_nodes_tensor: torch.Tensor, max_sample_counts,
                      random_seeds=None, *, wm_csr_weight_ptr_tensor=None, need_edge_ids: bool = False,
                      wm_edge_attr_tensors=None):
    """Extension (wholememory_ext_multilayer_sample): every hop of an unweighted multi-layer sample in ONE library call with no
    host round trip inside — buffers sized for their upper bounds, counts kept on the device between hops, ONE stream
    synchronise here at the end. Returns a list with one (sample_offset, unique, neighbor_pos, center_lid, edge_index) tuple per
    hop, hop 0 next to the seeds, each tensor trimmed to its size and equal to what `sample_append_unique` returns hop by hop
    with the same seeds — or None when the library declines (see multilayer_sample_begin): run hop by hop then.
    wm_csr_weight_ptr_tensor (keyword): the weighted sampler on these edge weights, see multilayer_sample_begin.
    need_edge_ids / wm_edge_attr_tensors (keyword): a sixth entry per hop, the int64 graph edge ids of the samples, and a
    seventh, the list of the given edge attributes at those edges; see multilayer_sample_begin."""
    pending = multilayer_sample_begin(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, seed_nodes_tensor, max_sample_counts,
                                      random_seeds, wm_csr_weight_ptr_tensor=wm_csr_weight_ptr_tensor,
                                      need_edge_ids=need_edge_ids, wm_edge_attr_tensors=wm_edge_attr_tensors)
    return None if pending is None else pending.finish()


def _is_distributed(h):
    L = wmb.lib()
    return bool(L.wholememory_tensor_has_handle(h)) and \
        L.wholememory_get_memory_type(C.c_void_p(L.wholememory_tensor_get_memory_handle(h))) == wmb.MT_DISTRIBUTED


def _weighted_sample_via_gather(row, col, wgt, center_nodes_tensor, max_sample_count, random_seed):
    """Weighted sampling where csr_row_ptr / csr_col_ptr or the weights are DISTRIBUTED, from the ops that reach such tensors.
    The unweighted sampler with max_sample_count -1 brings every neighbour of the centres in row order (on a DISTRIBUTED graph
    through its gather route) with its edge id; a gather brings their weights; those three arrays are a CSR graph on this
    device whose node i is centre i, and the weighted sampler runs on it. Its keys depend on the seed, on a centre's position
    in the batch and on a neighbour's position in its row, all unchanged, so the samples are those of a mapped graph.
    Collective (every rank calls it, with its own centres); it moves the centres' whole rows.
    -> (sample_offset, sampled node ids, center local id, edge id)"""
    from .tensor import WholeMemoryTensor
    if random_seed is None:
        random_seed = random.getrandbits(64)
    desc = wmb.lib().wholememory_tensor_get_tensor_description
    if _tensor_dim(wgt) != 1 or int(desc(wgt).contents.sizes[0]) != int(desc(col).contents.sizes[0]):
        wmb.check(6, "wm_csr_weight_ptr_tensor must have one weight per edge")      # WHOLEMEMORY_INVALID_INPUT
    offset, neighbours, edge_id = unweighted_sample_without_replacement(row, col, center_nodes_tensor, -1, 0, False, True)
    weights = WholeMemoryTensor(wgt).gather(edge_id)
    n = center_nodes_tensor.shape[0]
    if edge_id.shape[0] == 0:      # (no centre, or none with a neighbour: offset is n + 1 zeros)
        return (offset, neighbours, torch.empty(0, device=op_device(), dtype=torch.int),
                torch.empty(0, device=op_device(), dtype=torch.int64))
    local = [wrap_torch_tensor(t) for t in (offset.to(torch.int64), neighbours, weights)]
    centres = torch.arange(n, device=center_nodes_tensor.device, dtype=center_nodes_tensor.dtype)
    offset, ids, lid, local_edge = weighted_sample_without_replacement(*[w.handle for w in local], centres, max_sample_count,
                                                                       random_seed, True, True)
    return offset, ids, lid, edge_id[local_edge]


def weighted_sample_without_replacement(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor,
                                        center_nodes_tensor: torch.Tensor, max_sample_count: int,
                                        random_seed: Union[int, None] = None, need_center_local_output: bool = False,
                                        need_edge_output: bool = False):
    """A-Res weighted sampling: neighbours are kept with probability proportional to their edge weight
    (wm_csr_weight_ptr_tensor: float32/float64, one per edge). max_sample_count <= 8192.
    A graph or weight tensor that is DISTRIBUTED (extension; the C entry point answers NOT_IMPLEMENTED) is sampled through
    `_weighted_sample_via_gather`: a collective, the same samples as on a mapped graph."""
    row, col, wgt = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor), _handle(wm_csr_weight_ptr_tensor)
    assert center_nodes_tensor.dim() == 1
    if any(_is_distributed(h) for h in (row, col, wgt)):
        out = _weighted_sample_via_gather(row, col, wgt, center_nodes_tensor, max_sample_count, random_seed)
        return out[:2] + ((out[2],) if need_center_local_output else ()) + ((out[3],) if need_edge_output else ())
    offset = torch.empty(center_nodes_tensor.shape[0] + 1, device=op_device(), dtype=torch.int)
    dest = TorchMemoryContext()
    lid = TorchMemoryContext() if need_center_local_output else None
    egid = TorchMemoryContext() if need_edge_output else None
    wc, wo = wrap_torch_tensor(center_nodes_tensor), wrap_torch_tensor(offset)
    wmb.check(wmb.lib().wholegraph_csr_weighted_sample_without_replacement(
        row, col, wgt, wc.handle, int(max_sample_count), wo.handle, C.c_void_p(dest.get_c_context()),
        C.c_void_p(lid.get_c_context() if lid else 0), C.c_void_p(egid.get_c_context() if egid else 0),
        _seed64(random_seed), get_wholegraph_env_fns(), C.c_void_p(get_stream())))
    return _sample_outputs(offset, dest, lid, egid, need_center_local_output, need_edge_output)


def _check_walk_arguments(start_nodes_tensor, walk_length):
    if int(walk_length) < 1:
        raise ValueError("walk_length must be at least 1, got %r" % (walk_length,))
    if start_nodes_tensor.dim() != 1:
        raise ValueError("start_nodes_tensor must be 1-D, got %d dimensions" % start_nodes_tensor.dim())


def _walk(entry, wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_weight_ptr_tensor, start_nodes_tensor, walk_length,
          step_rule, random_seed, need_edge_output):
    """The library call of random_walk and node2vec_walk. `entry` takes the graph, the starts and the length, then
    `step_rule` (the step rule's own arguments: none for random_walk), then the seed, the two outputs and the stream."""
    row, col = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor)
    wgt = None if wm_csr_weight_ptr_tensor is None else _handle(wm_csr_weight_ptr_tensor)
    n, steps = start_nodes_tensor.shape[0], int(walk_length)
    walks = torch.empty((n, steps + 1), device=op_device(), dtype=_col_dtype(col))
    edge_ids = torch.empty((n, steps), device=op_device(), dtype=torch.int64) if need_edge_output else None
    ws, ww = wrap_torch_tensor(start_nodes_tensor), wrap_torch_tensor(walks)
    we = wrap_torch_tensor(edge_ids) if need_edge_output else None
    wmb.check(entry(row, col, wgt, ws.handle, steps, *step_rule, _seed64(random_seed), ww.handle,
                    we.handle if we is not None else None, C.c_void_p(get_stream())))
    return (walks, edge_ids) if need_edge_output else walks


def random_walk(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, start_nodes_tensor: torch.Tensor, walk_length: int,
                random_seed: Union[int, None] = None, *, wm_csr_weight_ptr_tensor=None, need_edge_output: bool = False):
    """Extension (wholememory_ext_csr_random_walk, include/wholememory/wholegraph_amd_ext.h section 2m): one random walk of
    `walk_length` steps from every start node, as ONE launch with no host round trip. Returns walks [n, walk_length + 1] in
    csr_col_ptr's dtype — column 0 the start node, -1 from the step at which a walk ends (no neighbour to go to, a start
    outside the graph) — or (walks, edge_ids) with need_edge_output: int64 [n, walk_length], the position in csr_col_ptr of
    every step taken, -1 elsewhere. A step goes to a neighbour picked uniformly, or, with wm_csr_weight_ptr_tensor (keyword;
    float32 / float64, one per edge), with probability proportional to its weight among the neighbours of positive weight.
    Walk w depends on (random_seed, w) alone, not on the size of the batch."""
    _check_walk_arguments(start_nodes_tensor, walk_length)
    return _walk(wmb.lib().wholememory_ext_csr_random_walk, wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor,
                 wm_csr_weight_ptr_tensor, start_nodes_tensor, walk_length, (), random_seed, need_edge_output)


def node2vec_walk(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, start_nodes_tensor: torch.Tensor, walk_length: int, p: float,
                  q: float, random_seed: Union[int, None] = None, *, wm_csr_weight_ptr_tensor=None, col_sorted: bool = False,
                  need_edge_output: bool = False):
    """Extension (wholememory_ext_csr_node2vec_walk, include/wholememory/wholegraph_amd_ext.h section 2n): one node2vec walk
    of `walk_length` steps from every start node, as ONE launch with no host round trip. Outputs as `random_walk`. From the
    second step on, the weight of a neighbour x of the current node (1 without wm_csr_weight_ptr_tensor) is multiplied by
    1 / p when x is the previous node, by 1 when x is a neighbour of the previous node, and by 1 / q otherwise; p = q = 1 gives
    the walks of `random_walk` with the same weights. col_sorted=True promises that every row of csr_col_ptr is ascending,
    and the neighbour test becomes a binary search instead of a scan of the previous node's row."""
    _check_walk_arguments(start_nodes_tensor, walk_length)
    for name, value in (("p", p), ("q", q)):
        if not (math.isfinite(float(value)) and float(value) > 0):
            raise ValueError("%s must be finite and positive, got %r" % (name, value))
    step_rule = (C.c_float(float(p)), C.c_float(float(q)), 1 if col_sorted else 0)
    return _walk(wmb.lib().wholememory_ext_csr_node2vec_walk, wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor,
                 wm_csr_weight_ptr_tensor, start_nodes_tensor, walk_length, step_rule, random_seed, need_edge_output)


NEGATIVE_MODES = {"uniform": 0, "degree": 1}


def negative_sample(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, src_nodes_tensor: torch.Tensor, num_negatives: int,
                    random_seed: Union[int, None] = None, *, mode: str = "uniform", exclude_edges: bool = True,
                    exclude_self: bool = True, max_tries: int = 8, col_sorted: bool = False):
    """Extension (wholememory_ext_csr_negative_sample, include/wholememory/wholegraph_amd_ext.h section 2o): for every source
    node `num_negatives` nodes that are not its neighbours (exclude_edges) and not the node itself (exclude_self), as ONE
    launch with no host round trip -> [n, num_negatives] in csr_col_ptr's dtype. mode "uniform" draws over the nodes, "degree"
    in proportion to how often a node occurs in csr_col_ptr. A sample takes at most `max_tries` (1 .. 64) draws and is -1 when
    all were rejected, or when the source is not a node; samples are drawn with replacement. col_sorted=True promises that
    every row of csr_col_ptr is ascending, and the neighbour test becomes a binary search instead of a scan of the row."""
    if int(num_negatives) < 1:
        raise ValueError("num_negatives must be at least 1, got %r" % (num_negatives,))
    if not 1 <= int(max_tries) <= 64:
        raise ValueError("max_tries must lie in 1 .. 64, got %r" % (max_tries,))
    if mode not in NEGATIVE_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(NEGATIVE_MODES), mode))
    if src_nodes_tensor.dim() != 1:
        raise ValueError("src_nodes_tensor must be 1-D, got %d dimensions" % src_nodes_tensor.dim())
    row, col = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor)
    n, k = src_nodes_tensor.shape[0], int(num_negatives)
    negatives = torch.empty((n, k), device=op_device(), dtype=_col_dtype(col))
    ws, wn = wrap_torch_tensor(src_nodes_tensor), wrap_torch_tensor(negatives)
    wmb.check(wmb.lib().wholememory_ext_csr_negative_sample(
        row, col, ws.handle, k, NEGATIVE_MODES[mode], (1 if exclude_edges else 0) | (2 if exclude_self else 0), int(max_tries),
        1 if col_sorted else 0, _seed64(random_seed), wn.handle, C.c_void_p(get_stream())))
    return negatives


def induced_subgraph(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, nodes_tensor: torch.Tensor, *, need_edge_output: bool = False):
    """Extension (wholememory_ext_csr_induced_subgraph, include/wholememory/wholegraph_amd_ext.h section 2q): every graph edge
    among `nodes` as one local CSR block, the batch of subgraph-wise training. Returns (offsets int32 [n + 1], col int32 [m][,
    edge ids int64 [m]]): row i lists, in the graph's order, the entries of row nodes[i] whose node occurs in `nodes`, each as
    the lowest position it occurs at; the edge ids are their positions in csr_col_ptr. Nodes outside the graph get empty rows
    and are never referred to; duplicates get a row each. One host round trip, for m."""
    if nodes_tensor.dim() != 1:
        raise ValueError("nodes_tensor must be 1-D, got %d dimensions" % nodes_tensor.dim())
    row, col = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor)
    offset = torch.empty(nodes_tensor.shape[0] + 1, device=op_device(), dtype=torch.int)
    out_col = TorchMemoryContext()
    egid = TorchMemoryContext() if need_edge_output else None
    wn, wo = wrap_torch_tensor(nodes_tensor), wrap_torch_tensor(offset)
    wmb.check(wmb.lib().wholememory_ext_csr_induced_subgraph(
        row, col, wn.handle, wo.handle, C.c_void_p(out_col.get_c_context()), C.c_void_p(egid.get_c_context() if egid else 0),
        get_wholegraph_env_fns(), C.c_void_p(get_stream())))
    if need_edge_output:
        return offset, out_col.get_tensor(), egid.get_tensor()
    return offset, out_col.get_tensor()


TEMPORAL_STRATEGIES = {"uniform": 0, "last": 1}
TEMPORAL_MAX_FANOUT = 64


def _check_temporal_arguments(center_nodes_tensor, center_times_tensor, max_sample_count, strategy, time_window):
    """-> (strategy code, time_window as the C ABI takes it: -1 for None)"""
    if strategy not in TEMPORAL_STRATEGIES:
        raise ValueError("strategy must be one of %s, got %r" % (sorted(TEMPORAL_STRATEGIES), strategy))
    if int(max_sample_count) > TEMPORAL_MAX_FANOUT:
        raise ValueError("max_sample_count must be at most %d, got %r" % (TEMPORAL_MAX_FANOUT, max_sample_count))
    if time_window is not None and not 0 <= int(time_window) < (1 << 63):
        raise ValueError("time_window must be None or lie in [0, 2^63), got %r" % (time_window,))
    if center_nodes_tensor.dim() != 1 or center_times_tensor.dim() != 1:
        raise ValueError("center_nodes_tensor and center_times_tensor must be 1-D")
    if center_times_tensor.shape[0] != center_nodes_tensor.shape[0]:
        raise ValueError("center_times_tensor must have one time per centre, got %d for %d centres"
                         % (center_times_tensor.shape[0], center_nodes_tensor.shape[0]))
    if center_times_tensor.dtype != torch.int64:
        raise ValueError("center_times_tensor must be int64, got %s" % center_times_tensor.dtype)
    return TEMPORAL_STRATEGIES[strategy], -1 if time_window is None else int(time_window)


def _temporal_sample_via_gather(row, col, tim, center_nodes_tensor, center_times_tensor, max_sample_count, random_seed, rule):
    """Temporal sampling where the graph or the time tensor is DISTRIBUTED, as `_weighted_sample_via_gather`: the unweighted
    sampler with max_sample_count -1 brings every neighbour of the centres in row order with its edge id, a gather brings
    their times, and the op runs on those three arrays as a device CSR whose node i is centre i. A centre's position in the
    batch and a neighbour's position in its row are unchanged, so the samples are those of a mapped graph. Collective.
    -> (sample_offset, sampled node ids, center local id, edge id)"""
    from .tensor import WholeMemoryTensor
    desc = wmb.lib().wholememory_tensor_get_tensor_description
    if _tensor_dim(tim) != 1 or int(desc(tim).contents.sizes[0]) != int(desc(col).contents.sizes[0]):
        wmb.check(6, "wm_csr_edge_time_tensor must have one timestamp per edge")      # WHOLEMEMORY_INVALID_INPUT
    if wholememory_dtype_to_torch_dtype(desc(tim).contents.dtype) != torch.int64:      # (before any collective work)
        wmb.check(3, "wm_csr_edge_time_tensor must be int64")      # WHOLEMEMORY_LOGIC_ERROR
    # the unweighted sampler reads the row bounds of whatever id it is given: a centre that is no node (an empty row here) is
    # fetched as node 0 and handed to the op below as centre -1, which is no node of the gathered rows either
    n = center_nodes_tensor.shape[0]
    is_node = (center_nodes_tensor >= 0) & (center_nodes_tensor < int(desc(row).contents.sizes[0]) - 1)
    fetched = torch.where(is_node, center_nodes_tensor, torch.zeros_like(center_nodes_tensor))
    offset, neighbours, edge_id = unweighted_sample_without_replacement(row, col, fetched, -1, 0, False, True)
    times = WholeMemoryTensor(tim).gather(edge_id)
    if edge_id.shape[0] == 0:      # (no centre, or none with a neighbour: offset is n + 1 zeros)
        return (offset, neighbours, torch.empty(0, device=op_device(), dtype=torch.int),
                torch.empty(0, device=op_device(), dtype=torch.int64))
    local = [wrap_torch_tensor(t) for t in (offset.to(torch.int64), neighbours, times)]
    centres = torch.arange(n, device=center_nodes_tensor.device, dtype=center_nodes_tensor.dtype)
    centres = torch.where(is_node, centres, torch.full_like(centres, -1))
    offset, ids, lid, local_edge = _temporal_sample_mapped(*[w.handle for w in local], centres, center_times_tensor,
                                                           max_sample_count, random_seed, True, True, rule)
    return offset, ids, lid, edge_id[local_edge]


def _temporal_sample_mapped(row, col, tim, center_nodes_tensor, center_times_tensor, max_sample_count, random_seed,
                            need_center_local_output, need_edge_output, rule):
    offset = torch.empty(center_nodes_tensor.shape[0] + 1, device=op_device(), dtype=torch.int)
    dest = TorchMemoryContext()
    lid = TorchMemoryContext() if need_center_local_output else None
    egid = TorchMemoryContext() if need_edge_output else None
    wc, wt, wo = wrap_torch_tensor(center_nodes_tensor), wrap_torch_tensor(center_times_tensor), wrap_torch_tensor(offset)
    strategy, inclusive, window = rule
    wmb.check(wmb.lib().wholememory_ext_csr_temporal_sample(
        row, col, tim, wc.handle, wt.handle, int(max_sample_count), strategy, 1 if inclusive else 0, C.c_longlong(window),
        _seed64(random_seed), wo.handle, C.c_void_p(dest.get_c_context()), C.c_void_p(lid.get_c_context() if lid else 0),
        C.c_void_p(egid.get_c_context() if egid else 0), get_wholegraph_env_fns(), C.c_void_p(get_stream())))
    return _sample_outputs(offset, dest, lid, egid, need_center_local_output, need_edge_output)


def temporal_sample_without_replacement(wm_csr_row_ptr_tensor, wm_csr_col_ptr_tensor, wm_csr_edge_time_tensor,
                                        center_nodes_tensor: torch.Tensor, center_times_tensor: torch.Tensor,
                                        max_sample_count: int, random_seed: Union[int, None] = None,
                                        need_center_local_output: bool = False, need_edge_output: bool = False, *,
                                        strategy: str = "uniform", inclusive: bool = True, time_window: Union[int, None] = None):
    """Extension (wholememory_ext_csr_temporal_sample, include/wholememory/wholegraph_amd_ext.h section 2r): for centre i — the
    node center_nodes_tensor[i] at the time center_times_tensor[i] (int64) — the neighbours whose edge time
    (wm_csr_edge_time_tensor: int64, one per edge) is not later than that time (earlier, with inclusive=False) and, with
    time_window, at most time_window before it; min(eligible, max_sample_count) of them, all eligible ones when
    max_sample_count <= 0. max_sample_count <= 64. strategy "uniform" keeps a uniform sample without replacement, "last" the
    latest edges; either way a centre's neighbours come in row order. Returns what the other samplers return:
    (sample_offset int32 [n + 1], sampled node ids[, center local id int32][, edge id int64]). Centre i's samples depend on
    (random_seed, i) and its row alone, not on the size of the batch. One host round trip, for the total.
    A graph or time tensor that is DISTRIBUTED (the C entry point answers NOT_IMPLEMENTED) is sampled through
    `_temporal_sample_via_gather`: a collective, the same samples as on a mapped graph."""
    code, window = _check_temporal_arguments(center_nodes_tensor, center_times_tensor, max_sample_count, strategy, time_window)
    rule = (code, bool(inclusive), window)
    row, col, tim = _handle(wm_csr_row_ptr_tensor), _handle(wm_csr_col_ptr_tensor), _handle(wm_csr_edge_time_tensor)
    if random_seed is None:
        random_seed = random.getrandbits(64)
    if any(_is_distributed(h) for h in (row, col, tim)):
        out = _temporal_sample_via_gather(row, col, tim, center_nodes_tensor, center_times_tensor, max_sample_count, random_seed, rule)
        return out[:2] + ((out[2],) if need_center_local_output else ()) + ((out[3],) if need_edge_output else ())
    return _temporal_sample_mapped(row, col, tim, center_nodes_tensor, center_times_tensor, max_sample_count, random_seed,
                                   need_center_local_output, need_edge_output, rule)


def generate_random_positive_int_cpu(random_seed, sub_sequence, output_random_value_count):
    output = torch.empty((output_random_value_count,), dtype=torch.int)
    w = wrap_torch_tensor(output)
    wmb.check(wmb.lib().generate_random_positive_int_cpu(int(random_seed), int(sub_sequence), w.handle))
    return output


def generate_exponential_distribution_negative_float_cpu(random_seed: int, sub_sequence: int,
                                                         output_random_value_count: int):
    output = torch.empty((output_random_value_count,), dtype=torch.float)
    w = wrap_torch_tensor(output)
    wmb.check(wmb.lib().generate_exponential_distribution_negative_float_cpu(int(random_seed), int(sub_sequence),
                                                                             w.handle))
    return output
