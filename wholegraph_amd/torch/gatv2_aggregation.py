"""GATv2 ("dynamic") multi-head graph attention over a sampled CSC block — the ``mha_gat_v2_n2n`` op behind the GATv2
layer (``wholememory_ext_csc_gatv2_forward`` / ``_backward``, kernels in ``csrc/kernels/gatv2.hip``).

``mha_gat_v2_n2n(h_src, h_dst, att, row_ptr, col_ind, heads)`` takes ``h_src = lin_src(x)`` as ``[n_src, H*F]``,
``h_dst = lin_dst(x[:n_dst])`` as ``[>= n_dst, H*F]`` (row ``d`` belongs to target ``d``; head ``k`` owns the columns
``[k*F, (k+1)*F)``) and ``att`` as ``[H*F]``, viewed as ``(H, F)``. Per target and head, an edge softmax of
``att . LeakyReLU(h_src[src] + h_dst[dst])`` weights the neighbour rows of ``h_src``: the non-linearity sits inside the
dot product, so the logit is one dot product over F per edge and head. Every fp32 sum, forward and backward, is taken in
one fixed order (stated in ``include/wholememory/wholegraph_amd_ext.h``, section 2g), so results are bitwise reproducible.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region 16-bit ``h_src`` / ``h_dst`` (what an autocast ``Linear``
returns) are cast to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast a 16-bit input is a
``TypeError``."""
import torch

from .aggregation import _block, _call, _opt_ptr, _ptr, _rows, _stride, _widen


class CscGatV2Conv(torch.autograd.Function):
    """autograd over the two entry points: out (and alpha, which carries no gradient) from h_src, h_dst and att"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, h_src, h_dst, att, row_ptr, col_ind, heads, negative_slope, concat):
        n_src, hf = h_src.shape
        dim = hf // heads
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        out = torch.empty((n_dst, hf if concat else dim), dtype=torch.float32, device=h_src.device)
        alpha = torch.empty((n_edges, heads), dtype=torch.float32, device=h_src.device)
        _call("csc_gatv2_forward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _ptr(h_src), _stride(h_src, hf),
              _ptr(h_dst), _stride(h_dst, hf), _ptr(att), heads, dim, float(negative_slope), int(bool(concat)), _ptr(out),
              out.shape[1], _ptr(alpha))
        ctx.save_for_backward(h_src, h_dst, att, row_ptr, col_ind, alpha)
        ctx.conf = (heads, dim, float(negative_slope), bool(concat))
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out, grad_alpha):
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return (None,) * 8
        h_src, h_dst, att, row_ptr, col_ind, alpha = ctx.saved_tensors
        heads, dim, slope, concat = ctx.conf
        n_src, hf = h_src.shape
        n_dst = row_ptr.shape[0] - 1
        grad_out = _rows(grad_out, "grad_out")
        dev = h_src.device
        grad_h_src = torch.empty((n_src, hf), dtype=torch.float32, device=dev) if need[0] else None
        # (rows of h_dst behind the targets take no part in the op: their gradient is zero)
        grad_h_dst = torch.zeros((h_dst.shape[0], hf), dtype=torch.float32, device=dev) if need[1] else None
        grad_att = torch.empty((hf,), dtype=torch.float32, device=dev) if need[2] else None
        _call("csc_gatv2_backward", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(h_src),
              _stride(h_src, hf), _ptr(h_dst), _stride(h_dst, hf), _ptr(att), heads, dim, slope, int(concat), _ptr(alpha),
              _ptr(grad_out), _stride(grad_out, grad_out.shape[1]), _opt_ptr(grad_h_src), hf, _opt_ptr(grad_h_dst), hf,
              _opt_ptr(grad_att))
        return grad_h_src, grad_h_dst, grad_att, None, None, None, None, None


def mha_gat_v2_n2n(h_src: torch.Tensor, h_dst: torch.Tensor, att: torch.Tensor, csr_row_ptr: torch.Tensor,
                   csr_col_ind: torch.Tensor, heads: int, negative_slope: float = 0.2, concat: bool = True,
                   return_alpha: bool = False):
    """GATv2 attention aggregation of a sampled block. h_src: fp32 [n_src, heads * F]; h_dst: fp32 [>= n_dst, heads * F],
    row d the target d (its first n_dst rows are used); att: fp32 [heads * F]; csr_row_ptr [n_dst + 1] and csr_col_ind [E]
    (int32 or int64, converted to int32): the edges of target d are csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]].
    Returns [n_dst, heads * F] with concat, else the mean over heads [n_dst, F]; with return_alpha also the attention
    weights alpha [E, heads] (no gradient flows through them)."""
    heads = int(heads)
    if heads < 1:
        raise ValueError("heads must be >= 1 (got %d)" % heads)
    h_src = _rows(_widen(h_src), "h_src")
    h_dst = _rows(_widen(h_dst), "h_dst")
    if not h_src.is_cuda:
        raise ValueError("h_src must be a GPU tensor")
    if h_src.shape[1] < 1 or h_src.shape[1] % heads:
        raise ValueError("h_src has %d columns: not a positive multiple of heads = %d" % (h_src.shape[1], heads))
    if h_dst.device != h_src.device or h_dst.shape[1] != h_src.shape[1]:
        raise ValueError("h_dst must have the %d columns of h_src and live on %s" % (h_src.shape[1], h_src.device))
    if att.dtype != torch.float32 or att.numel() != h_src.shape[1] or att.device != h_src.device:
        raise ValueError("att must be fp32 with heads * F = %d elements on %s" % (h_src.shape[1], h_src.device))
    att = att.reshape(-1).contiguous()
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, h_src.device, h_src=h_src, h_dst=h_dst)
    out, alpha = CscGatV2Conv.apply(h_src, h_dst, att, row_ptr, col_ind, heads, float(negative_slope), bool(concat))
    return (out, alpha) if return_alpha else out
