"""Multi-aggregator neighbour aggregation of a sampled CSC block — the ``agg_concat_pna`` op behind the PNAConv layer
(``wholememory_ext_csc_pna_aggregate_forward`` / ``_backward``, kernels in ``csrc/kernels/pna.hip``).

``agg_concat_pna(x, row_ptr, col_ind, aggregators)`` returns ``[n_dst, (A + 1) * F]``: one slot of ``F`` columns per selected
aggregator, always in the order ``sum, mean, min, max, std`` whatever order ``aggregators`` lists them in, then the target's
own row (the targets are the first ``n_dst`` rows of ``x``, as for ``agg_concat``). Every neighbour row is read once for all
of them. ``std`` is ``sqrt(max(E[x^2] - E[x]^2, 0) + eps)``; a target without edges gets +0.0 in every aggregator slot.
``min`` / ``max`` give a tie to the lowest edge position, and so does their gradient. Every fp32 operation, forward and
backward, is taken in one fixed order (stated in ``include/wholememory/wholegraph_amd_ext.h``, section 2l), so results are
bitwise reproducible. With ``["max"]`` alone the op is GraphSAGE's max aggregation.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region a 16-bit ``x`` (what an autocast ``Linear`` returns) is cast
to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast a 16-bit or float64 ``x`` is a
``TypeError``."""
import torch

from .. import binding as wmb
from .aggregation import _block, _call, _opt_ptr, _ptr, _rows, _stride, _widen

AGGREGATORS = tuple(wmb.PNA_AGGR)   # canonical (slot) order
EPS = 1e-5


def aggregator_mask(aggregators) -> int:
    """the 5-bit mask of the C ABI from a non-empty list of distinct names out of sum / mean / min / max / std"""
    if isinstance(aggregators, str):
        aggregators = [aggregators]
    names = list(aggregators)
    if not names:
        raise ValueError("aggregators must name at least one of %s" % ", ".join(AGGREGATORS))
    mask = 0
    for name in names:
        if name not in wmb.PNA_AGGR:
            raise ValueError("unknown aggregator %r (one of %s)" % (name, ", ".join(AGGREGATORS)))
        if mask & wmb.PNA_AGGR[name]:
            raise ValueError("aggregator %r is listed twice" % (name,))
        mask |= wmb.PNA_AGGR[name]
    return mask


def aggregator_names(mask: int):
    """the selected names in slot order"""
    return [n for n in AGGREGATORS if mask & wmb.PNA_AGGR[n]]


class CscAggregatePNA(torch.autograd.Function):
    """autograd over the two entry points; what the backward needs from the forward (the arg rows of min / max, mean and
    coefficient of std) is allocated, and written, only when x needs a gradient (`save`)"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, row_ptr, col_ind, mask, eps, save):
        n_src, dim = x.shape
        n_dst = row_ptr.shape[0] - 1
        slots = bin(mask).count("1") + 1
        out = torch.empty((n_dst, slots * dim), dtype=torch.float32, device=x.device)
        saved = [None] * 4   # arg_min, arg_max, std_mean, std_coef
        if save:   # (decided by the caller: grad mode is off in here whatever it was outside)
            for i, (bit, dt) in enumerate(((4, torch.int32), (8, torch.int32), (16, torch.float32), (16, torch.float32))):
                if mask & bit:
                    saved[i] = torch.empty((n_dst, dim), dtype=dt, device=x.device)
        _call("csc_pna_aggregate_forward", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(x),
              _stride(x, dim), dim, mask, eps, _ptr(out), slots * dim, *map(_opt_ptr, saved), lib=wmb.lib())
        ctx.save_for_backward(x if mask & 16 else None, row_ptr, col_ind, *saved)
        ctx.conf = (n_src, dim, mask)
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        x, row_ptr, col_ind, *saved = ctx.saved_tensors
        n_src, dim, mask = ctx.conf
        n_dst = row_ptr.shape[0] - 1
        slots = bin(mask).count("1") + 1
        grad_out = _rows(grad_out, "grad_out")
        grad_x = torch.empty((n_src, dim), dtype=torch.float32, device=grad_out.device)
        _call("csc_pna_aggregate_backward", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _opt_ptr(x),
              _stride(x, dim) if x is not None else dim, dim, mask, *map(_opt_ptr, saved), _ptr(grad_out),
              _stride(grad_out, slots * dim), _ptr(grad_x), dim, lib=wmb.lib())
        return grad_x, None, None, None, None, None


def agg_concat_pna(x: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor,
                   aggregators=("mean", "min", "max", "std"), eps: float = EPS) -> torch.Tensor:
    """[n_dst, (A + 1) * F] = (the selected aggregators over each target's neighbour rows of x, in the order sum, mean, min,
    max, std; the target's own row). csr_row_ptr [n_dst + 1] and csr_col_ind [E] (int32 or int64, converted to int32)
    describe the block in CSC form: the edges of target d are csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]], row
    positions in x. x: float32 [n_src, F], n_src >= n_dst. aggregators: a non-empty list of distinct names."""
    mask = aggregator_mask(aggregators)
    x = _rows(_widen(x), "x")
    if not x.is_cuda:
        raise ValueError("x must be a GPU tensor")
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, x.device, x=x)
    if x.shape[1] < 1:
        raise ValueError("x needs at least one column")
    if not eps >= 0:
        raise ValueError("eps must be >= 0 (got %r)" % (eps,))
    save = torch.is_grad_enabled() and x.requires_grad
    return CscAggregatePNA.apply(x, row_ptr, col_ind, mask, float(eps), save)
