"""Edge-weighted neighbour aggregation of a sampled CSC block — ``agg_concat`` with one fp32 weight per edge
(``wholememory_ext_csc_aggregate_weighted_forward`` / ``_weighted_backward``, kernels in ``csrc/kernels/agg_weighted.hip``).

``agg_concat_weighted(x, row_ptr, col_ind, edge_weight, aggr)`` returns ``[n_dst, 2F]``: the sum (or, for ``"mean"``, the
sum divided by the target's DEGREE — DGL's edge-weight convention, not the weighted average) of ``edge_weight[e] *
x[col_ind[e]]`` over each target's edges, then the target's own row. Gradients flow into ``x`` and into ``edge_weight``;
only the one that is asked for is computed. Every fp32 sum, forward and backward, is taken in one fixed order (stated in
``include/wholememory/wholegraph_amd_ext.h``, section 2d), every product is rounded before the add that follows it, and
there are no atomics: results are bitwise reproducible.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region a 16-bit ``x`` (what an autocast ``Linear`` returns) is
cast to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast a 16-bit ``x`` is a ``TypeError``."""
import torch

from .aggregation import _block, _call, _opt_ptr, _ptr, _rows, _stride, _widen, aggr_code

# what the backward calls asked the library for, newest last: (grad_x computed, grad_w computed). A gradient that autograd
# does not need is passed as a null pointer and nothing is queued for it; tests read this to see that.
backward_requests = []
_MAX_REQUESTS = 64


class CscAggregateConcatWeighted(torch.autograd.Function):
    """autograd over the two entry points; x is kept for the backward only when the weights can ask for a gradient"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, row_ptr, col_ind, aggr_code_):
        n_src, dim = x.shape
        n_dst = row_ptr.shape[0] - 1
        out = torch.empty((n_dst, 2 * dim), dtype=torch.float32, device=x.device)
        _call("csc_aggregate_weighted_forward", _ptr(row_ptr), _ptr(col_ind), _ptr(w), col_ind.shape[0], n_dst, n_src,
              _ptr(x), _stride(x, dim), dim, aggr_code_, _ptr(out), _stride(out, 2 * dim))
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.save_for_backward(row_ptr, col_ind, w if (want_x or want_w) else None, x if want_w else None)
        ctx.shape = (n_src, dim)
        ctx.aggr = aggr_code_
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_w):
            return None, None, None, None, None
        row_ptr, col_ind, w, x = ctx.saved_tensors
        n_src, dim = ctx.shape
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        grad_out = _rows(grad_out, "grad_out")
        grad_x = torch.empty((n_src, dim), dtype=torch.float32, device=grad_out.device) if want_x else None
        # (a block without targets has no edge of any target: nothing is written then)
        grad_w = (torch.empty if n_dst else torch.zeros)((n_edges,), dtype=torch.float32, device=grad_out.device) \
            if want_w else None
        if grad_x is None and n_edges == 0:   # (only the gradient of no weight at all is asked for)
            return None, grad_w, None, None, None
        _call("csc_aggregate_weighted_backward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _opt_ptr(x),
              _stride(x, dim) if x is not None else dim, _ptr(w), _ptr(grad_out), _stride(grad_out, 2 * dim), dim, ctx.aggr,
              _opt_ptr(grad_x), dim, _opt_ptr(grad_w))
        backward_requests.append((grad_x is not None, grad_w is not None))
        del backward_requests[:-_MAX_REQUESTS]
        return grad_x, grad_w, None, None, None


def agg_concat_weighted(x: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor, edge_weight: torch.Tensor,
                        aggr: str = "mean") -> torch.Tensor:
    """[n_dst, 2F] = (aggr over each target's edges of edge_weight[e] * x[csr_col_ind[e]], the target's own row).
    csr_row_ptr [n_dst + 1] and csr_col_ind [E] (int32 or int64, converted to int32) describe the block in CSC form as for
    agg_concat; edge_weight: float32 [E], one weight per entry of csr_col_ind. x: float32 [n_src, F], n_src >= n_dst.
    "mean" divides the weighted sum by the target's degree. Differentiable in x and in edge_weight."""
    code = aggr_code(aggr)
    x = _rows(_widen(x), "x")
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, x.device, x=x)
    if edge_weight.dtype != torch.float32:
        raise TypeError("edge_weight must be float32 (got %s)" % edge_weight.dtype)
    if edge_weight.dim() != 1:
        raise ValueError("edge_weight must be 1-D (got shape %s)" % (tuple(edge_weight.shape),))
    if edge_weight.device != x.device:
        raise ValueError("edge_weight is on %s, x on %s" % (edge_weight.device, x.device))
    if edge_weight.shape[0] != col_ind.shape[0]:
        raise ValueError("edge_weight has %d entries, csr_col_ind %d" % (edge_weight.shape[0], col_ind.shape[0]))
    if x.shape[1] < 1:
        raise ValueError("x needs at least one column")
    if not x.is_cuda:
        raise ValueError("x must be a GPU tensor")
    return CscAggregateConcatWeighted.apply(x, edge_weight.contiguous(), row_ptr, col_ind, code)
