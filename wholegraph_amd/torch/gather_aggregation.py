"""``agg_concat`` straight from a WholeMemory table — layer 0 of a GNN without the gathered ``[n_src, F]`` intermediate
(``wholememory_ext_csc_gather_aggregate_forward``, kernel in ``csrc/kernels/agg_gather.hip``).

``gather_agg_concat(source, node_ids, row_ptr, col_ind, aggr)`` returns what
``agg_concat(source.gather(node_ids, force_dtype=torch.float32), row_ptr, col_ind, aggr)`` returns, bit for bit: float32
``[n_dst, 2F]``, the sum (or mean) of each target's neighbour rows in the fixed order stated in
``include/wholememory/wholegraph_amd_ext.h`` (section 2e), then the target's own row. ``source`` is a
``WholeMemoryEmbedding`` or a ``WholeMemoryTensor`` of float32, float16 or bfloat16 rows; 16-bit rows are widened (exactly)
as they are read. Every id must be a row of the table: there is no "skip me" id here.

The fused kernel reads CONTINUOUS and CHUNKED tables, the types that are mapped into the calling process. Any other table
(DISTRIBUTED, HIERARCHY), an embedding with a cache policy and any other dtype take the two-op composition instead, with
identical results; ``calls()`` counts the fused forwards and so tells the routes apart.

Training follows ``EmbeddingLookupFn``'s contract: when ``source`` is an embedding with an optimizer and ``is_training``
is set, the backward computes the gradient of the (virtual) gathered rows with the fp32 ``agg_concat`` backward, hands
``(node_ids, grad_x)`` to the embedding and marks it for the next ``WholeMemoryOptimizer.step``. Otherwise the backward
queues no work: for frozen features nothing needs those rows.

``source`` may also be a ``WholeMemoryQuantizedTensor`` (8-bit row-quantized features, ``quantized``): the result then
equals ``agg_concat(source.gather(node_ids), row_ptr, col_ind, aggr)`` bit for bit. A CONTINUOUS or CHUNKED quantized table
in device memory is read by one kernel (``wholememory_ext_csc_gather_dequantize_aggregate_forward``, kernel in
``csrc/kernels/agg_quant.hip``) that dequantizes the rows as it adds them; ``quantized_calls()`` counts those forwards. A
host-located table takes the composition (the fused kernel would pull a row across PCIe once per edge, the gather pulls
each of the n_src rows once), as do DISTRIBUTED and HIERARCHY tables. Quantized tables are frozen features: the output
carries no autograd node and ``is_training`` is ignored."""
import torch

from .. import binding as wmb
from .aggregation import _block, _call, _ptr, _rows, _stride, agg_concat, aggr_code
from .embedding import EmbeddingLookupFn, WholeMemoryEmbedding
from .quantized import WholeMemoryQuantizedTensor
from .tensor import WholeMemoryTensor
from .wholegraph_env import op_device

_TABLE_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_ID_DTYPES = {torch.int32: wmb.DT_INT, torch.int64: wmb.DT_INT64}


def calls() -> int:
    """fused forwards that reached the device backend in this process"""
    return int(wmb.lib().wholememory_ext_gather_aggregate_calls())


def quantized_calls() -> int:
    """fused forwards over a quantized table that launched on the device backend in this process"""
    return int(wmb.lib().wholememory_ext_gather_dequantize_aggregate_calls())


def _table_of(source) -> WholeMemoryTensor:
    """the WholeMemoryTensor behind `source` (of a quantized source: its int8 storage)"""
    if isinstance(source, WholeMemoryEmbedding):
        return source.get_embedding_tensor()
    if isinstance(source, WholeMemoryTensor):
        return source
    if isinstance(source, WholeMemoryQuantizedTensor):
        return source.storage
    raise TypeError("source must be a WholeMemoryEmbedding, a WholeMemoryTensor or a WholeMemoryQuantizedTensor (got %s)"
                    % type(source).__name__)


def takes_fused_route(source) -> bool:
    """True when gather_agg_concat(source, ...) runs the fused kernel: a float32 / float16 / bfloat16 table of a mapped
    type (continuous, chunked) that is not behind a cache policy; or a quantized table of such a type in device memory"""
    table = _table_of(source)
    if isinstance(source, WholeMemoryQuantizedTensor):
        L = wmb.lib()
        return (L.wholememory_get_memory_type(table._handle()) in (wmb.MT_CONTINUOUS, wmb.MT_CHUNKED)
                and L.wholememory_get_memory_location(table._handle()) == wmb.ML_DEVICE)
    if isinstance(source, WholeMemoryEmbedding) and source.wmb_cache_policy is not None:
        return False
    if table.dim() != 2 or table.dtype not in _TABLE_DTYPES:
        return False
    return wmb.lib().wholememory_get_memory_type(table._handle()) in (wmb.MT_CONTINUOUS, wmb.MT_CHUNKED)


class GatherAggregateConcat(torch.autograd.Function):
    """autograd over the fused forward. `dummy_input` is the embedding's anchor (EmbeddingLookupFn): the only
    differentiable input, so that autograd calls the backward, which hands the row gradients to the embedding."""

    @staticmethod
    def forward(ctx, node_ids, dummy_input, source, table, row_ptr, col_ind, aggr_code_, is_training):
        n_src, dim = node_ids.shape[0], table.shape[1]
        n_dst = row_ptr.shape[0] - 1
        out = torch.empty((n_dst, 2 * dim), dtype=torch.float32, device=node_ids.device)
        _call("csc_gather_aggregate_forward", table.wmb_tensor, _ptr(node_ids), _ID_DTYPES[node_ids.dtype], _ptr(row_ptr),
              _ptr(col_ind), col_ind.shape[0], n_dst, n_src, aggr_code_, _ptr(out), 2 * dim)
        trains = isinstance(source, WholeMemoryEmbedding) and source.wmb_optimizer is not None and bool(is_training)
        ctx.target = source if trains else None
        ctx.dummy_like = (tuple(dummy_input.shape), dummy_input.dtype, dummy_input.device)
        if trains:
            ctx.save_for_backward(node_ids, row_ptr, col_ind)
            ctx.dim = dim
            ctx.aggr = aggr_code_
        return out

    @staticmethod
    def backward(ctx, grad_out):
        target, ctx.target = ctx.target, None
        if target is None:   # frozen features: nothing to do, for anybody
            return None, None, None, None, None, None, None, None
        node_ids, row_ptr, col_ind = ctx.saved_tensors
        n_src, dim = node_ids.shape[0], ctx.dim
        n_dst = row_ptr.shape[0] - 1
        grad_out = _rows(grad_out, "grad_out")
        grad_x = torch.empty((n_src, dim), dtype=torch.float32, device=grad_out.device)
        _call("csc_aggregate_backward_typed", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(grad_out),
              _stride(grad_out, 2 * dim), dim, ctx.aggr, _ptr(grad_x), dim, wmb.DT_FLOAT, what="csc_aggregate_backward")
        target.add_gradients(node_ids, grad_x)
        target.need_apply = True
        shape, dtype, device = ctx.dummy_like
        return None, torch.zeros(shape, dtype=dtype, device=device), None, None, None, None, None, None


def _quantized_forward(source, node_ids, row_ptr, col_ind, aggr_code_):
    n_src, dim = node_ids.shape[0], source.shape[1]
    n_dst = row_ptr.shape[0] - 1
    out = torch.empty((n_dst, 2 * dim), dtype=torch.float32, device=node_ids.device)
    _call("csc_gather_dequantize_aggregate_forward", source.storage.wmb_tensor, dim, _ptr(node_ids),
          _ID_DTYPES[node_ids.dtype], _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, aggr_code_, _ptr(out),
          2 * dim)
    return out


def gather_agg_concat(source, node_ids: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor,
                      aggr: str = "mean", *, is_training: bool = False) -> torch.Tensor:
    """float32 [n_dst, 2F] = (aggr over each target's neighbour rows, the target's own row), the rows being
    source[node_ids[i]] widened to float32: node_ids [n_src] (int32 or int64, on the GPU) are the global ids of the block's
    nodes, targets first, as append_unique leaves them; csr_row_ptr [n_dst + 1] and csr_col_ind [E] as for agg_concat.
    The rows of a WholeMemoryQuantizedTensor are dequantized as they are read."""
    code = aggr_code(aggr)
    table = _table_of(source)
    if node_ids.dim() != 1:
        raise ValueError("node_ids must be 1-D")
    if node_ids.dtype not in _ID_DTYPES:
        raise TypeError("node_ids must be int32 or int64 (got %s)" % node_ids.dtype)
    quantized = isinstance(source, WholeMemoryQuantizedTensor)
    if quantized and csr_row_ptr.shape[0] - 1 > node_ids.shape[0]:   # (the same refusal on both routes)
        raise ValueError("more targets (%d) than node ids (%d)" % (csr_row_ptr.shape[0] - 1, node_ids.shape[0]))
    if not takes_fused_route(source):
        if quantized:
            x = source.gather(node_ids)
        elif isinstance(source, WholeMemoryEmbedding):
            x = EmbeddingLookupFn.apply(node_ids, source.dummy_input, source, is_training, torch.float32)
        else:
            x = table.gather(node_ids, force_dtype=torch.float32)
        return agg_concat(x, csr_row_ptr, csr_col_ind, aggr)
    if not node_ids.is_cuda:
        node_ids = node_ids.to(op_device())
    node_ids = node_ids.contiguous()
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, node_ids.device)
    if row_ptr.shape[0] - 1 > node_ids.shape[0]:
        raise ValueError("more targets (%d) than node ids (%d)" % (row_ptr.shape[0] - 1, node_ids.shape[0]))
    if table.shape[1] < 1:
        raise ValueError("the table needs at least one column")
    if quantized:   # frozen features: no autograd node, nothing to run backwards
        return _quantized_forward(source, node_ids, row_ptr, col_ind, code)
    dummy = source.dummy_input if isinstance(source, WholeMemoryEmbedding) else torch.zeros(1)
    return GatherAggregateConcat.apply(node_ids, dummy, source, table, row_ptr, col_ind, code, is_training)
