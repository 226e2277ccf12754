"""Multi-head graph attention over a sampled CSC block — the ``mha_gat_n2n`` op behind the GAT layer
(``wholememory_ext_csc_gat_forward`` / ``_backward``, kernels in ``csrc/kernels/gat.hip``).

``mha_gat_n2n(h, att, row_ptr, col_ind, heads)`` takes ``h = lin(x)`` as ``[n_src, H*F]`` (head ``k`` owns the columns
``[k*F, (k+1)*F)``; the targets are the first ``n_dst`` rows) and ``att`` as ``[2*H*F]``, viewed as ``(2, H, F)``: half 0
the source (neighbour) side, half 1 the target side. Per target and head, an edge softmax of
``LeakyReLU(att[0] . h[src] + att[1] . h[dst])`` weights the neighbour rows. Every fp32 sum, forward and backward, is
taken in one fixed order (stated in ``include/wholememory/wholegraph_amd_ext.h``, section 2c), so results are bitwise
reproducible.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region a 16-bit ``h`` (what an autocast ``Linear`` returns) is
cast to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast a 16-bit ``h`` is a ``TypeError``."""
import torch

from .. import binding as wmb
from .aggregation import _block, _call, _ptr, _rows, _stride, _widen


def node_chunk() -> int:
    """N: the backward sums grad_att over chunks of this many node rows (the chunk sums added in chunk order)"""
    return int(wmb.lib().wholememory_ext_csc_gat_node_chunk())


class CscGatConv(torch.autograd.Function):
    """autograd over the two entry points: out (and alpha, which carries no gradient) from h and att"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, h, att, row_ptr, col_ind, heads, negative_slope, concat):
        n_src, hf = h.shape
        dim = hf // heads
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        out = torch.empty((n_dst, hf if concat else dim), dtype=torch.float32, device=h.device)
        alpha = torch.empty((n_edges, heads), dtype=torch.float32, device=h.device)
        scores = torch.empty((n_src + n_dst, heads), dtype=torch.float32, device=h.device)
        _call("csc_gat_forward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _ptr(h), _stride(h, hf), _ptr(att),
              heads, dim, float(negative_slope), int(bool(concat)), _ptr(out), out.shape[1], _ptr(alpha), _ptr(scores))
        ctx.save_for_backward(h, att, row_ptr, col_ind, alpha, scores)
        ctx.conf = (heads, dim, float(negative_slope), bool(concat))
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out, grad_alpha):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None, None, None
        h, att, row_ptr, col_ind, alpha, scores = ctx.saved_tensors
        heads, dim, slope, concat = ctx.conf
        n_src, hf = h.shape
        n_dst = row_ptr.shape[0] - 1
        grad_out = _rows(grad_out, "grad_out")
        grad_h = torch.empty((n_src, hf), dtype=torch.float32, device=h.device)
        grad_att = torch.empty((2 * hf,), dtype=torch.float32, device=h.device)
        _call("csc_gat_backward", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(h), _stride(h, hf),
              _ptr(att), heads, dim, slope, int(concat), _ptr(alpha), _ptr(scores), _ptr(grad_out),
              _stride(grad_out, grad_out.shape[1]), _ptr(grad_h), hf, _ptr(grad_att))
        return (grad_h if ctx.needs_input_grad[0] else None, grad_att if ctx.needs_input_grad[1] else None,
                None, None, None, None, None)


def mha_gat_n2n(h: torch.Tensor, att: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor, heads: int,
                negative_slope: float = 0.2, concat: bool = True, return_alpha: bool = False):
    """GAT attention aggregation of a sampled block. h: fp32 [n_src, heads * F] (the targets are its first n_dst rows);
    att: fp32 [2 * heads * F] ((2, heads, F): source half, then target half); csr_row_ptr [n_dst + 1] and csr_col_ind [E]
    (int32 or int64, converted to int32): the edges of target d are csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]].
    Returns [n_dst, heads * F] with concat, else the mean over heads [n_dst, F]; with return_alpha also the attention
    weights alpha [E, heads] (no gradient flows through them)."""
    heads = int(heads)
    if heads < 1:
        raise ValueError("heads must be >= 1 (got %d)" % heads)
    h = _rows(_widen(h), "h")
    if not h.is_cuda:
        raise ValueError("h must be a GPU tensor")
    if h.shape[1] < 1 or h.shape[1] % heads:
        raise ValueError("h has %d columns: not a positive multiple of heads = %d" % (h.shape[1], heads))
    if att.dtype != torch.float32 or att.numel() != 2 * h.shape[1] or att.device != h.device:
        raise ValueError("att must be fp32 with 2 * heads * F = %d elements on %s" % (2 * h.shape[1], h.device))
    att = att.reshape(-1).contiguous()
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, h.device, h=h)
    out, alpha = CscGatConv.apply(h, att, row_ptr, col_ind, heads, float(negative_slope), bool(concat))
    return (out, alpha) if return_alpha else out
