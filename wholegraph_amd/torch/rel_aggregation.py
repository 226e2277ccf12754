"""Relation-typed neighbour aggregation of a sampled CSC block — ``agg_concat`` with one relation per edge and one output
slot per relation, the aggregation behind the RGCN layer (``wholememory_ext_csc_rel_aggregate_forward`` / ``_backward``,
kernels in ``csrc/kernels/agg_rel.hip``).

``agg_concat_rel(x, row_ptr, col_ind, edge_type, num_relations, aggr)`` returns ``[n_dst, (R + 1) * F]``: for each relation
``r`` the sum (or, for ``"mean"``, the mean over the edges OF THAT RELATION — the RGCN paper's ``c_{i,r}``, PyG's default) of
``x[col_ind[e]]`` over the target's edges with ``edge_type[e] == r``, ``+0.0`` where a target has no such edge, then the
target's own row. An edge whose type is outside ``[0, R)`` contributes nothing, forward or backward. Gradients flow into
``x``. Every fp32 sum, forward and backward, is taken in one fixed order (stated in
``include/wholememory/wholegraph_amd_ext.h``, section 2h), every product is rounded before the add that follows it, and
there are no atomics: results are bitwise reproducible.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region a 16-bit ``x`` (what an autocast ``Linear`` returns) is
cast to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast a 16-bit ``x`` is a ``TypeError``."""
import torch

from .. import binding as wmb
from .aggregation import _block, _call, _opt_ptr, _ptr, _rows, _stride, _widen, aggr_code


class CscAggregateConcatRel(torch.autograd.Function):
    """autograd over the two entry points; x is not kept for the backward (the per-edge scale of "mean" is)"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, row_ptr, col_ind, edge_type, num_relations, aggr_code_):
        n_src, dim = x.shape
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        width = (num_relations + 1) * dim
        out = torch.empty((n_dst, width), dtype=torch.float32, device=x.device)
        # (a block without targets has no edge of any target: nothing is written then)
        scale = (torch.empty if n_dst else torch.zeros)((n_edges,), dtype=torch.float32, device=x.device) \
            if aggr_code_ == wmb.AGGR_MEAN else None
        _call("csc_rel_aggregate_forward", _ptr(row_ptr), _ptr(col_ind), _ptr(edge_type), n_edges, n_dst, n_src,
              num_relations, _ptr(x), _stride(x, dim), dim, aggr_code_, _ptr(out), _stride(out, width), _opt_ptr(scale))
        ctx.save_for_backward(row_ptr, col_ind, edge_type, scale)
        ctx.shape = (n_src, dim)
        ctx.num_relations = num_relations
        ctx.aggr = aggr_code_
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        row_ptr, col_ind, edge_type, scale = ctx.saved_tensors
        n_src, dim = ctx.shape
        n_dst = row_ptr.shape[0] - 1
        width = (ctx.num_relations + 1) * dim
        grad_out = _rows(grad_out, "grad_out")
        grad_x = torch.empty((n_src, dim), dtype=torch.float32, device=grad_out.device)
        _call("csc_rel_aggregate_backward", _ptr(row_ptr), _ptr(col_ind), _ptr(edge_type), col_ind.shape[0], n_dst, n_src,
              ctx.num_relations, _opt_ptr(scale), _ptr(grad_out), _stride(grad_out, width), dim, ctx.aggr, _ptr(grad_x), dim)
        return grad_x, None, None, None, None, None


def _edge_types(t: torch.Tensor, num_relations: int, device) -> torch.Tensor:
    """int32 types; an int64 type that int32 cannot hold becomes -1 (out of range either way) instead of wrapping round"""
    if t.dim() != 1:
        raise ValueError("edge_type must be 1-D (got shape %s)" % (tuple(t.shape),))
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError("edge_type must be int32 or int64 (got %s)" % t.dtype)
    if t.device != device:
        raise ValueError("edge_type is on %s, x on %s" % (t.device, device))
    if t.dtype == torch.int64:
        t = torch.where((t < 0) | (t >= num_relations), -1, t).to(torch.int32)
    return t.contiguous()


def agg_concat_rel(x: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor, edge_type: torch.Tensor,
                   num_relations: int, aggr: str = "mean") -> torch.Tensor:
    """[n_dst, (R + 1) * F] = (for r < R: aggr over the target's edges of relation r of x[csr_col_ind[e]], the target's own
    row). csr_row_ptr [n_dst + 1] and csr_col_ind [E] (int32 or int64, converted to int32) describe the block in CSC form as
    for agg_concat; edge_type: int32 or int64 [E], the relation of each entry of csr_col_ind (a value outside [0, R)
    contributes nothing). x: float32 [n_src, F], n_src >= n_dst. "mean" divides a slot's sum by the number of the target's
    edges of that relation. Differentiable in x."""
    code = aggr_code(aggr)
    if isinstance(num_relations, bool) or not isinstance(num_relations, int):
        raise TypeError("num_relations must be an int (got %s)" % type(num_relations).__name__)
    if num_relations < 1:
        raise ValueError("num_relations must be >= 1 (got %d)" % num_relations)
    x = _rows(_widen(x), "x")
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, x.device, x=x)
    types = _edge_types(edge_type, num_relations, x.device)
    if types.shape[0] != col_ind.shape[0]:
        raise ValueError("edge_type has %d entries, csr_col_ind %d" % (types.shape[0], col_ind.shape[0]))
    if x.shape[1] < 1:
        raise ValueError("x needs at least one column")
    if not x.is_cuda:
        raise ValueError("x must be a GPU tensor")
    return CscAggregateConcatRel.apply(x, row_ptr, col_ind, types, num_relations, code)
