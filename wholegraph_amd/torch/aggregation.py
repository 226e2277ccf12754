"""Neighbour aggregation of a sampled CSC block — the ``agg_concat`` op behind the GraphSAGE layer
(``wholememory_ext_csc_aggregate_forward_typed`` / ``_backward_typed``, kernels in ``csrc/kernels/agg.hip`` for fp32 rows
and ``csrc/kernels/agg_half.hip`` for fp16 / bf16 rows).

``agg_concat(x, row_ptr, col_ind, aggr)`` returns ``[n_dst, 2F]``: the sum (or mean) of each target's neighbour rows of
``x``, then the target's own row (the targets are the first ``n_dst`` rows of ``x``, as ``append_unique`` leaves them).
Every fp32 sum, forward and backward, is taken in one fixed order (stated in ``include/wholememory/wholegraph_amd_ext.h``),
so results are bitwise reproducible.

``x`` may be float32, float16 or bfloat16; ``out`` and the gradient of ``x`` have its dtype. With 16-bit rows the sums are
still taken in fp32, in the same order, and each output element is rounded once (to nearest even): the result equals the
fp32 op on ``x.float()`` rounded to ``x.dtype``, bit for bit. The op has no autocast rule of its own: inside
``torch.autocast`` it runs in the dtype its input arrives in, so a layer fed by an autocast ``Linear`` aggregates 16-bit
rows and one fed by fp32 features aggregates fp32 rows."""
import ctypes as C

import torch

from .. import binding as wmb
from .wholegraph_env import get_stream, get_wholegraph_env_fns

_AGGR = {"sum": wmb.AGGR_SUM, "mean": wmb.AGGR_MEAN}
_ROW_DTYPES = {torch.float32: wmb.DT_FLOAT, torch.float16: wmb.DT_HALF, torch.bfloat16: wmb.DT_BF16}


def aggr_code(aggr: str) -> int:
    if aggr in ("max", "min"):
        raise NotImplementedError("aggr=%r: only 'mean' and 'sum' are implemented" % aggr)
    if aggr not in _AGGR:
        raise ValueError("aggr must be 'mean' or 'sum' (got %r)" % (aggr,))
    return _AGGR[aggr]


def chunk_edges() -> int:
    """C: a source's edges are summed in chunks of this many by the backward (the chunk sums added in chunk order)"""
    return int(wmb.lib().wholememory_ext_csc_aggregate_chunk_edges())


def _rows(t: torch.Tensor, what: str, dtypes=(torch.float32,)) -> torch.Tensor:
    """a 2-D tensor of one of `dtypes` whose rows are unit-stride (a row stride of its own is fine)"""
    if t.dtype not in dtypes:
        raise TypeError("%s must be %s (got %s)" % (what, " or ".join(str(d).replace("torch.", "") for d in dtypes), t.dtype))
    if t.dim() != 2:
        raise ValueError("%s must be 2-D (got shape %s)" % (what, tuple(t.shape)))
    if (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _index(t: torch.Tensor, what: str, device) -> torch.Tensor:
    if t.dim() != 1:
        raise ValueError("%s must be 1-D" % what)
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError("%s must be int32 or int64 (got %s)" % (what, t.dtype))
    if t.device != device:
        raise ValueError("%s is on %s, x on %s" % (what, t.device, device))
    return t.to(torch.int32).contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _opt_ptr(t):
    """None stays None: the null pointer of a tensor that is left out"""
    return _ptr(t) if t is not None else None


def _stride(t: torch.Tensor, width: int) -> int:
    """the row stride the library is told: a tensor without rows has none worth trusting, so the width of a row"""
    return t.stride(0) if t.shape[0] else width


def _widen(t: torch.Tensor) -> torch.Tensor:
    """what custom_fwd's cast_inputs does, ahead of the dtype checks of an fp32-only op: inside autocast a 16-bit GPU
    tensor is widened"""
    if t.is_cuda and t.dtype in (torch.float16, torch.bfloat16) and torch.is_autocast_enabled("cuda"):
        return t.float()
    return t


def _block(csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor, device, **rows):
    """(row_ptr, col_ind) as int32 on `device`; every tensor of `rows` (by the name the caller's signature gives it) holds a
    row per target"""
    row_ptr = _index(csr_row_ptr, "csr_row_ptr", device)
    col_ind = _index(csr_col_ind, "csr_col_ind", device)
    if row_ptr.shape[0] < 1:
        raise ValueError("csr_row_ptr needs n_dst + 1 >= 1 entries")
    for name, t in rows.items():
        if row_ptr.shape[0] - 1 > t.shape[0]:
            raise ValueError("more targets (%d) than rows of %s (%d)" % (row_ptr.shape[0] - 1, name, t.shape[0]))
    return row_ptr, col_ind


def _call(entry: str, *args, what: str = None, lib=None):
    """wholememory_ext_<entry>(*args, env functions, stream), checked; `what` names the call in the error, `lib` is the
    library handle of a module that resolves its own (pna_aggregation: its tests watch the calls through it)"""
    fn = getattr(lib if lib is not None else wmb.lib(), "wholememory_ext_" + entry)
    wmb.check(fn(*args, get_wholegraph_env_fns(), C.c_void_p(get_stream())), what or entry)


class CscAggregateConcat(torch.autograd.Function):
    """autograd over the two entry points; the edge index of the backward is built only when x needs a gradient (the
    backward runs only then)"""

    @staticmethod
    def forward(ctx, x, row_ptr, col_ind, aggr_code_):
        n_src, dim = x.shape
        n_dst = row_ptr.shape[0] - 1
        out = torch.empty((n_dst, 2 * dim), dtype=x.dtype, device=x.device)
        _call("csc_aggregate_forward_typed", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(x),
              _stride(x, dim), dim, aggr_code_, _ptr(out), _stride(out, 2 * dim), _ROW_DTYPES[x.dtype],
              what="csc_aggregate_forward")
        ctx.save_for_backward(row_ptr, col_ind)
        ctx.shape = (n_src, dim)
        ctx.dtype = x.dtype
        ctx.aggr = aggr_code_
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        row_ptr, col_ind = ctx.saved_tensors
        n_src, dim = ctx.shape
        n_dst = row_ptr.shape[0] - 1
        grad_out = _rows(grad_out, "grad_out", (ctx.dtype,))   # (autograd hands over the dtype of out)
        grad_x = torch.empty((n_src, dim), dtype=ctx.dtype, device=grad_out.device)
        _call("csc_aggregate_backward_typed", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(grad_out),
              _stride(grad_out, 2 * dim), dim, ctx.aggr, _ptr(grad_x), dim, _ROW_DTYPES[ctx.dtype],
              what="csc_aggregate_backward")
        return grad_x, None, None, None


def agg_concat(x: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor, aggr: str = "mean") -> torch.Tensor:
    """[n_dst, 2F] = (aggr over each target's neighbour rows of x, the target's own row). csr_row_ptr [n_dst + 1] and
    csr_col_ind [E] (int32 or int64, converted to int32) describe the block in CSC form: the edges of target d are
    csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]], row positions in x. x: float32, float16 or bfloat16 [n_src, F],
    n_src >= n_dst; the result has x's dtype (16-bit rows: fp32 sums, one rounding per element)."""
    code = aggr_code(aggr)
    x = _rows(x, "x", tuple(_ROW_DTYPES))
    if not x.is_cuda:
        raise ValueError("x must be a GPU tensor")
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, x.device, x=x)
    if x.shape[1] < 1:
        raise ValueError("x needs at least one column")
    return CscAggregateConcat.apply(x, row_ptr, col_ind, code)
