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
import ctypes as C

import torch

from .. import binding as wmb
from .aggregation import _index, _ptr, _rows, aggr_code
from .wholegraph_env import get_stream, get_wholegraph_env_fns

# what the backward calls asked the library for, newest last: (grad_x computed, grad_w computed). A gradient that autograd
# does not need is passed as a null pointer and nothing is queued for it; tests read this to see that.
backward_requests = []
_MAX_REQUESTS = 64


def _opt_ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


class CscAggregateConcatWeighted(torch.autograd.Function):
    """autograd over the two entry points; x is kept for the backward only when the weights can ask for a gradient"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, row_ptr, col_ind, aggr_code_):
        n_src, dim = x.shape
        n_dst = row_ptr.shape[0] - 1
        out = torch.empty((n_dst, 2 * dim), dtype=torch.float32, device=x.device)
        wmb.check(wmb.lib().wholememory_ext_csc_aggregate_weighted_forward(
            _ptr(row_ptr), _ptr(col_ind), _ptr(w), col_ind.shape[0], n_dst, n_src, _ptr(x), x.stride(0) if n_src else dim,
            dim, aggr_code_, _ptr(out), out.stride(0) if n_dst else 2 * dim, get_wholegraph_env_fns(),
            C.c_void_p(get_stream())), "csc_aggregate_weighted_forward")
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
        wmb.check(wmb.lib().wholememory_ext_csc_aggregate_weighted_backward(
            _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _opt_ptr(x),
            x.stride(0) if (x is not None and n_src) else dim, _ptr(w), _ptr(grad_out),
            grad_out.stride(0) if n_dst else 2 * dim, dim, ctx.aggr, _opt_ptr(grad_x), dim, _opt_ptr(grad_w),
            get_wholegraph_env_fns(), C.c_void_p(get_stream())), "csc_aggregate_weighted_backward")
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
    if x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and torch.is_autocast_enabled("cuda"):
        x = x.float()   # (what custom_fwd's cast_inputs does, ahead of the checks below; the op is fp32)
    x = _rows(x, "x")
    row_ptr = _index(csr_row_ptr, "csr_row_ptr", x.device)
    col_ind = _index(csr_col_ind, "csr_col_ind", x.device)
    if edge_weight.dtype != torch.float32:
        raise TypeError("edge_weight must be float32 (got %s)" % edge_weight.dtype)
    if edge_weight.dim() != 1:
        raise ValueError("edge_weight must be 1-D (got shape %s)" % (tuple(edge_weight.shape),))
    if edge_weight.device != x.device:
        raise ValueError("edge_weight is on %s, x on %s" % (edge_weight.device, x.device))
    if edge_weight.shape[0] != col_ind.shape[0]:
        raise ValueError("edge_weight has %d entries, csr_col_ind %d" % (edge_weight.shape[0], col_ind.shape[0]))
    if row_ptr.shape[0] < 1:
        raise ValueError("csr_row_ptr needs n_dst + 1 >= 1 entries")
    if row_ptr.shape[0] - 1 > x.shape[0]:
        raise ValueError("more targets (%d) than rows of x (%d)" % (row_ptr.shape[0] - 1, x.shape[0]))
    if x.shape[1] < 1:
        raise ValueError("x needs at least one column")
    if not x.is_cuda:
        raise ValueError("x must be a GPU tensor")
    return CscAggregateConcatWeighted.apply(x, edge_weight.contiguous(), row_ptr, col_ind, code)
