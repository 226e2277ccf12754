"""Scaled dot-product multi-head attention over a sampled CSC block — the ``mha_simple_n2n`` op behind the TransformerConv
layer (``wholememory_ext_csc_mha_simple_forward`` / ``_backward``, kernels in ``csrc/kernels/tconv.hip``).

``mha_simple_n2n(key_emb, query_emb, value_emb, row_ptr, col_ind, heads)`` takes ``key_emb = lin_key(x)`` and
``value_emb = lin_value(x)`` as ``[n_src, H*F]`` and ``query_emb = lin_query(x[:n_dst])`` as ``[>= n_dst, H*F]`` (row ``d``
belongs to target ``d``; head ``k`` owns the columns ``[k*F, (k+1)*F)``). Per target and head, an edge softmax of
``query[dst] . key[src]`` (times ``1 / sqrt(F)`` with ``norm_by_dim``) weights the neighbour rows of ``value_emb``. Every
fp32 sum, forward and backward, is taken in one fixed order (stated in ``include/wholememory/wholegraph_amd_ext.h``, section
2k), so results are bitwise reproducible.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region 16-bit inputs (what an autocast ``Linear`` returns) are cast
to fp32 on the way in and the op runs in fp32 with autocast off; outside autocast a 16-bit input is a ``TypeError``."""
import torch

from .aggregation import _block, _call, _opt_ptr, _ptr, _rows, _stride, _widen


class CscMhaSimple(torch.autograd.Function):
    """autograd over the two entry points: out (and alpha, which carries no gradient) from key, query and value"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, key, query, value, row_ptr, col_ind, heads, concat, norm_by_dim):
        n_src, hf = key.shape
        dim = hf // heads
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        out = torch.empty((n_dst, hf if concat else dim), dtype=torch.float32, device=key.device)
        alpha = torch.empty((n_edges, heads), dtype=torch.float32, device=key.device)
        _call("csc_mha_simple_forward", _ptr(row_ptr), _ptr(col_ind), n_edges, n_dst, n_src, _ptr(key), _stride(key, hf),
              _ptr(query), _stride(query, hf), _ptr(value), _stride(value, hf), heads, dim, int(bool(norm_by_dim)),
              int(bool(concat)), _ptr(out), out.shape[1], _ptr(alpha))
        ctx.save_for_backward(key, query, value, row_ptr, col_ind, alpha)
        ctx.conf = (heads, dim, bool(concat), bool(norm_by_dim))
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_out, grad_alpha):
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return (None,) * 8
        key, query, value, row_ptr, col_ind, alpha = ctx.saved_tensors
        heads, dim, concat, norm_by_dim = ctx.conf
        n_src, hf = key.shape
        n_dst = row_ptr.shape[0] - 1
        grad_out = _rows(grad_out, "grad_out")
        dev = key.device
        grad_key = torch.empty((n_src, hf), dtype=torch.float32, device=dev) if need[0] else None
        # (rows of query behind the targets take no part in the op: their gradient is zero)
        grad_query = torch.zeros((query.shape[0], hf), dtype=torch.float32, device=dev) if need[1] else None
        grad_value = torch.empty((n_src, hf), dtype=torch.float32, device=dev) if need[2] else None
        _call("csc_mha_simple_backward", _ptr(row_ptr), _ptr(col_ind), col_ind.shape[0], n_dst, n_src, _ptr(key),
              _stride(key, hf), _ptr(query), _stride(query, hf), _ptr(value), _stride(value, hf), heads, dim,
              int(norm_by_dim), int(concat), _ptr(alpha), _ptr(grad_out), _stride(grad_out, grad_out.shape[1]),
              _opt_ptr(grad_key), hf, _opt_ptr(grad_query), hf, _opt_ptr(grad_value), hf)
        return grad_key, grad_query, grad_value, None, None, None, None, None


def mha_simple_n2n(key_emb: torch.Tensor, query_emb: torch.Tensor, value_emb: torch.Tensor, csr_row_ptr: torch.Tensor,
                   csr_col_ind: torch.Tensor, heads: int, concat: bool = True, norm_by_dim: bool = True,
                   return_alpha: bool = False):
    """Scaled dot-product attention aggregation of a sampled block. key_emb and value_emb: fp32 [n_src, heads * F];
    query_emb: fp32 [>= n_dst, heads * F], row d the target d (its first n_dst rows are used); csr_row_ptr [n_dst + 1] and
    csr_col_ind [E] (int32 or int64, converted to int32): the edges of target d are
    csr_col_ind[csr_row_ptr[d] : csr_row_ptr[d + 1]]. With norm_by_dim the logits are divided by sqrt(F). Returns
    [n_dst, heads * F] with concat, else the mean over heads [n_dst, F]; with return_alpha also the attention weights alpha
    [E, heads] (no gradient flows through them)."""
    heads = int(heads)
    if heads < 1:
        raise ValueError("heads must be >= 1 (got %d)" % heads)
    key = _rows(_widen(key_emb), "key_emb")
    query = _rows(_widen(query_emb), "query_emb")
    value = _rows(_widen(value_emb), "value_emb")
    if not key.is_cuda:
        raise ValueError("key_emb must be a GPU tensor")
    if key.shape[1] < 1 or key.shape[1] % heads:
        raise ValueError("key_emb has %d columns: not a positive multiple of heads = %d" % (key.shape[1], heads))
    if query.device != key.device or query.shape[1] != key.shape[1]:
        raise ValueError("query_emb must have the %d columns of key_emb and live on %s" % (key.shape[1], key.device))
    if value.device != key.device or value.shape[1] != key.shape[1]:
        raise ValueError("value_emb must have the %d columns of key_emb and live on %s" % (key.shape[1], key.device))
    if value.shape[0] != key.shape[0]:
        raise ValueError("value_emb has %d rows, key_emb %d" % (value.shape[0], key.shape[0]))
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, key.device, key_emb=key, query_emb=query)
    out, alpha = CscMhaSimple.apply(key, query, value, row_ptr, col_ind, heads, bool(concat), bool(norm_by_dim))
    return (out, alpha) if return_alpha else out
