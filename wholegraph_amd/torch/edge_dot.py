"""The dot product of the two endpoint rows of every edge of a sampled CSC block — the ``edge_dot_n2n`` op
(``wholememory_ext_csc_edge_dot_forward`` / ``_backward``, kernels in ``csrc/kernels/edot.hip``): the score of skip-gram
training over walks and negatives (``node2vec.py``) and the decoder of a link-prediction model over the GNN layers.

``edge_dot_n2n(x_src, x_dst, row_ptr, col_ind)`` returns ``[E]``: ``score[e] = x_dst[d] . x_src[col_ind[e]]`` for edge ``e``
of target ``d``. ``x_dst`` holds a row per target (``[>= n_dst, F]``) and is a tensor of its own: unlike the aggregation ops
the targets are not the first rows of ``x_src``, and there may be more of them than source rows. Every fp32 sum, forward and
backward, is taken in one fixed order (stated in ``include/wholememory/wholegraph_amd_ext.h``, section 2p) and nothing is
added atomically, so scores and both gradients are bitwise reproducible, where the composite
``(x_dst[dst] * x_src[col]).sum(-1)`` materialises two ``[E, F]`` tensors and adds its gradients in a different order from
run to run.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region 16-bit inputs are cast to fp32 on the way in and the op runs
in fp32 with autocast off; outside autocast a 16-bit input is a ``TypeError``."""
import torch

from .aggregation import _block, _call, _opt_ptr, _ptr, _rows, _stride, _widen


class CscEdgeDot(torch.autograd.Function):
    """autograd over the two entry points: needs_input_grad selects the gradients the backward computes"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x_src, x_dst, row_ptr, col_ind):
        n_src, dim = x_src.shape
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        score = torch.empty((n_edges,), dtype=torch.float32, device=x_src.device)
        _call("csc_edge_dot_forward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _ptr(x_src), _stride(x_src, dim),
              _ptr(x_dst), _stride(x_dst, dim), dim, _ptr(score))
        ctx.save_for_backward(x_src, x_dst, row_ptr, col_ind)
        return score

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_score):
        need = ctx.needs_input_grad[:2]
        if not any(need):
            return None, None, None, None
        x_src, x_dst, row_ptr, col_ind = ctx.saved_tensors
        n_src, dim = x_src.shape
        n_dst = row_ptr.shape[0] - 1
        grad_score = grad_score.contiguous()
        dev = x_src.device
        grad_src = torch.empty((n_src, dim), dtype=torch.float32, device=dev) if need[0] else None
        # (rows of x_dst behind the targets take no part in the op: their gradient is zero)
        grad_dst = torch.zeros((x_dst.shape[0], dim), dtype=torch.float32, device=dev) if need[1] else None
        _call("csc_edge_dot_backward", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(x_src),
              _stride(x_src, dim), _ptr(x_dst), _stride(x_dst, dim), dim, _ptr(grad_score), _opt_ptr(grad_src), dim,
              _opt_ptr(grad_dst), dim)
        return grad_src, grad_dst, None, None


def edge_dot_n2n(x_src: torch.Tensor, x_dst: torch.Tensor, csr_row_ptr: torch.Tensor, csr_col_ind: torch.Tensor) -> torch.Tensor:
    """[E] fp32: score[e] = x_dst[d] . x_src[csr_col_ind[e]] for every edge e of every target d. x_src: fp32 [n_src, F];
    x_dst: fp32 [>= n_dst, F], row d the target d (its first n_dst rows are used; n_dst may exceed n_src); csr_row_ptr
    [n_dst + 1] and csr_col_ind [E] (int32 or int64, converted to int32): the edges of target d are
    csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]], row positions in x_src. Gradients flow into both row tensors; the same
    tensor may be passed as both."""
    src = _rows(_widen(x_src), "x_src")
    dst = _rows(_widen(x_dst), "x_dst")
    if not src.is_cuda:
        raise ValueError("x_src must be a GPU tensor")
    if src.shape[1] < 1:
        raise ValueError("x_src needs at least one column")
    if dst.device != src.device or dst.shape[1] != src.shape[1]:
        raise ValueError("x_dst must have the %d columns of x_src and live on %s" % (src.shape[1], src.device))
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, src.device, x_dst=dst)
    return CscEdgeDot.apply(src, dst, row_ptr, col_ind)
