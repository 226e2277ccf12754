"""Multi-head graph attention over a sampled CSC block with edge features in the logit — ``mha_gat_n2n`` with cugraph-ops'
``edge_feat`` (``wholememory_ext_csc_gat_edge_forward`` / ``_backward``, kernels in ``csrc/kernels/gat_edge.hip``).

``mha_gat_n2n_edge(h, att, edge_feat, row_ptr, col_ind, heads)`` takes ``h = lin(x)`` as ``[n_src, H*F]`` and
``edge_feat = lin_edge(edge_attr)`` as ``[E, H*F]`` (row ``e`` belongs to edge position ``e`` of ``col_ind``; head ``k`` owns
the columns ``[k*F, (k+1)*F)`` of both), and ``att`` as ``[3*H*F]``, viewed as ``(3, H, F)``: half 0 the source side, half 1
the target side, half 2 the edge side. Per target and head, an edge softmax of
``LeakyReLU((att[0] . h[src] + att[1] . h[dst]) + att[2] . edge_feat[e])`` weights the neighbour rows ``h[src]``: the edge
features enter the logit only. Every fp32 sum, forward and backward, is taken in one fixed order (stated in
``include/wholememory/wholegraph_amd_ext.h``, section 2f), so results are bitwise reproducible; with ``edge_feat`` all zero
the op is ``gat_aggregation.mha_gat_n2n`` over ``att[:2*H*F]``, bit for bit.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region a 16-bit ``h`` / ``edge_feat`` (what an autocast ``Linear``
returns) is cast to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast it is a ``TypeError``."""
import torch

from .aggregation import _block, _call, _ptr, _rows, _stride, _widen
from .gat_aggregation import node_chunk  # noqa: F401  (N of grad_att's chunks: nodes for halves 0 and 1, edges for half 2)


class CscGatEdgeConv(torch.autograd.Function):
    """autograd over the two entry points: out (and alpha, which carries no gradient) from h, att and edge_feat"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, h, att, edge_feat, row_ptr, col_ind, heads, negative_slope, concat):
        n_src, hf = h.shape
        dim = hf // heads
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        out = torch.empty((n_dst, hf if concat else dim), dtype=torch.float32, device=h.device)
        alpha = torch.empty((n_edges, heads), dtype=torch.float32, device=h.device)
        scores = torch.empty((n_src + n_dst, heads), dtype=torch.float32, device=h.device)
        edge_scores = torch.empty((n_edges, heads), dtype=torch.float32, device=h.device)
        _call("csc_gat_edge_forward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _ptr(h), _stride(h, hf),
              _ptr(att), _ptr(edge_feat), _stride(edge_feat, hf), heads, dim, float(negative_slope), int(bool(concat)),
              _ptr(out), out.shape[1], _ptr(alpha), _ptr(scores), _ptr(edge_scores))
        ctx.save_for_backward(h, att, edge_feat, row_ptr, col_ind, alpha, scores, edge_scores)
        ctx.conf = (heads, dim, float(negative_slope), bool(concat))
        ctx.mark_non_differentiable(alpha, edge_scores)
        return out, alpha, edge_scores

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out, grad_alpha, grad_edge_scores):
        if not any(ctx.needs_input_grad[:3]):
            return (None,) * 8
        h, att, edge_feat, row_ptr, col_ind, alpha, scores, edge_scores = ctx.saved_tensors
        heads, dim, slope, concat = ctx.conf
        n_src, hf = h.shape
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        grad_out = _rows(grad_out, "grad_out")
        grad_h = torch.empty((n_src, hf), dtype=torch.float32, device=h.device)
        grad_att = torch.empty((3 * hf,), dtype=torch.float32, device=h.device)
        # (a block without targets has no edge of any target: nothing is written there)
        grad_ef = (torch.empty if n_dst else torch.zeros)((n_edges, hf), dtype=torch.float32, device=h.device)
        _call("csc_gat_edge_backward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _ptr(h), _stride(h, hf),
              _ptr(att), _ptr(edge_feat), _stride(edge_feat, hf), heads, dim, slope, int(concat), _ptr(alpha), _ptr(scores),
              _ptr(edge_scores), _ptr(grad_out), _stride(grad_out, grad_out.shape[1]), _ptr(grad_h), hf, _ptr(grad_att),
              _ptr(grad_ef), hf)
        return (grad_h if ctx.needs_input_grad[0] else None, grad_att if ctx.needs_input_grad[1] else None,
                grad_ef if ctx.needs_input_grad[2] else None, None, None, None, None, None)


def mha_gat_n2n_edge(h: torch.Tensor, att: torch.Tensor, edge_feat: torch.Tensor, csr_row_ptr: torch.Tensor,
                     csr_col_ind: torch.Tensor, heads: int, negative_slope: float = 0.2, concat: bool = True,
                     return_alpha: bool = False):
    """GAT attention aggregation of a sampled block with edge features in the logit. h: fp32 [n_src, heads * F] (the
    targets are its first n_dst rows); att: fp32 [3 * heads * F] ((3, heads, F): source, target, edge side); edge_feat: fp32
    [E, heads * F], row e for edge position e; csr_row_ptr [n_dst + 1] and csr_col_ind [E] (int32 or int64, converted to
    int32): the edges of target d are csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]].
    Returns [n_dst, heads * F] with concat, else the mean over heads [n_dst, F]; with return_alpha also the attention
    weights alpha [E, heads] (no gradient flows through them). CscGatEdgeConv.apply also returns the edge scores
    att[2] . edge_feat [E, heads]."""
    heads = int(heads)
    if heads < 1:
        raise ValueError("heads must be >= 1 (got %d)" % heads)
    h = _rows(_widen(h), "h")
    edge_feat = _rows(_widen(edge_feat), "edge_feat")
    if h.shape[1] < 1 or h.shape[1] % heads:
        raise ValueError("h has %d columns: not a positive multiple of heads = %d" % (h.shape[1], heads))
    if att.dtype != torch.float32 or att.numel() != 3 * h.shape[1] or att.device != h.device:
        raise ValueError("att must be fp32 with 3 * heads * F = %d elements on %s" % (3 * h.shape[1], h.device))
    if csr_col_ind.dim() != 1 or tuple(edge_feat.shape) != (csr_col_ind.shape[0], h.shape[1]):
        raise ValueError("edge_feat must be [E, heads * F] = [%d, %d] (got %s)" % (
            csr_col_ind.shape[0] if csr_col_ind.dim() == 1 else -1, h.shape[1], tuple(edge_feat.shape)))
    if not h.is_cuda:
        raise ValueError("h must be a GPU tensor")
    if edge_feat.device != h.device:
        raise ValueError("edge_feat is on %s, h on %s" % (edge_feat.device, h.device))
    att = att.reshape(-1).contiguous()
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, h.device, h=h)
    out, alpha, _ = CscGatEdgeConv.apply(h, att, edge_feat, row_ptr, col_ind, heads, float(negative_slope), bool(concat))
    return (out, alpha) if return_alpha else out
