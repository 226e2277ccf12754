"""The relation-typed score of every edge of a sampled CSC block — the ``kge_score_n2n`` op
(``wholememory_ext_csc_kge_score_forward`` / ``_backward``, kernels in ``csrc/kernels/kge.hip``): the decoder of the
knowledge-graph embedding models DistMult, TransE (l1 and l2), ComplEx and RotatE.

``kge_score_n2n(x_src, x_dst, rel, row_ptr, col_ind, edge_type, model=...)`` returns ``[E]`` fp32. The block is that of
``edge_dot_n2n``: ``x_dst`` holds a row per target and there may be more targets than source rows. Edge ``e`` of target ``d``
has the head ``x_dst[d]``, the tail ``x_src[col_ind[e]]`` (``head="src"``: the other way round) and the relation row
``rel[edge_type[e]]``. The complex models read a row as ``[re | im]``; for ``"rotate"`` the caller passes
``cat(cos(phase), sin(phase))`` as ``rel``. Every fp32 sum, forward and backward, is taken in one fixed order (stated in
``include/wholememory/wholegraph_amd_ext.h``, section 2u) and nothing is added atomically, so the scores and the three
gradients — into both row tensors and into the relation table — are bitwise reproducible, where the composite
``(x[h] * rel[type] * x[t]).sum(-1)`` materialises three ``[E, F]`` tensors and adds its gradients in a different order from
run to run.

The op is fp32 only. Inside a ``torch.autocast("cuda")`` region 16-bit inputs are cast to fp32 on the way in and the op runs
in fp32 with autocast off; outside autocast a 16-bit input is a ``TypeError``."""
import torch

from .aggregation import _block, _call, _index, _opt_ptr, _ptr, _rows, _stride, _widen

MODELS = {"distmult": 0, "transe_l1": 1, "transe_l2": 2, "complex": 3, "rotate": 4}
COMPLEX_MODELS = ("complex", "rotate")


class CscKgeScore(torch.autograd.Function):
    """autograd over the two entry points: needs_input_grad selects the gradients the backward computes"""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x_src, x_dst, rel, row_ptr, col_ind, edge_type, model, head_src):
        n_src, dim = x_src.shape
        n_dst, n_edges = row_ptr.shape[0] - 1, col_ind.shape[0]
        score = torch.empty((n_edges,), dtype=torch.float32, device=x_src.device)
        _call("csc_kge_score_forward", _ptr(row_ptr), _ptr(col_ind), _ptr(edge_type), n_edges, n_dst, n_src, rel.shape[0],
              _ptr(x_src), _stride(x_src, dim), _ptr(x_dst), _stride(x_dst, dim), _ptr(rel), _stride(rel, dim), dim, model,
              head_src, _ptr(score))
        ctx.save_for_backward(x_src, x_dst, rel, row_ptr, col_ind, edge_type, score)
        ctx.model, ctx.head_src = model, head_src
        return score

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_score):
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return (None,) * 8
        x_src, x_dst, rel, row_ptr, col_ind, edge_type, score = ctx.saved_tensors
        n_src, dim = x_src.shape
        n_dst = row_ptr.shape[0] - 1
        grad_score = grad_score.contiguous()
        dev = x_src.device
        grad_src = torch.empty((n_src, dim), dtype=torch.float32, device=dev) if need[0] else None
        # (rows of x_dst behind the targets take no part in the op: their gradient is zero)
        grad_dst = torch.zeros((x_dst.shape[0], dim), dtype=torch.float32, device=dev) if need[1] else None
        grad_rel = torch.empty((rel.shape[0], dim), dtype=torch.float32, device=dev) if need[2] else None
        _call("csc_kge_score_backward", _ptr(row_ptr), _ptr(col_ind), _ptr(edge_type), col_ind.shape[0], n_dst, n_src,
              rel.shape[0], _ptr(x_src), _stride(x_src, dim), _ptr(x_dst), _stride(x_dst, dim), _ptr(rel), _stride(rel, dim),
              dim, ctx.model, ctx.head_src, _ptr(score), _ptr(grad_score), _opt_ptr(grad_src), dim, _opt_ptr(grad_dst), dim,
              _opt_ptr(grad_rel), dim)
        return grad_src, grad_dst, grad_rel, None, None, None, None, None


def kge_score_n2n(x_src: torch.Tensor, x_dst: torch.Tensor, rel: torch.Tensor, csr_row_ptr: torch.Tensor,
                  csr_col_ind: torch.Tensor, edge_type: torch.Tensor, *, model: str, head: str = "dst") -> torch.Tensor:
    """[E] fp32: the score of every edge e of every target d under `model` ("distmult", "transe_l1", "transe_l2", "complex",
    "rotate"). x_src: fp32 [n_src, F]; x_dst: fp32 [>= n_dst, F], row d the target d (n_dst may exceed n_src); rel: fp32
    [R, F]; csr_row_ptr [n_dst + 1], csr_col_ind [E] and edge_type [E] int32 or int64 (converted to int32). head: "dst", the
    head of an edge is its target's row and the tail x_src[csr_col_ind[e]], or "src", the roles swapped. A type outside
    [0, R) scores +0.0 and contributes to no gradient. Gradients flow into x_src, x_dst and rel."""
    if model not in MODELS:
        raise ValueError("model must be one of %s (got %r)" % (", ".join(MODELS), model))
    if head not in ("dst", "src"):
        raise ValueError("head must be 'dst' or 'src' (got %r)" % (head,))
    src = _rows(_widen(x_src), "x_src")
    dst = _rows(_widen(x_dst), "x_dst")
    r = _rows(_widen(rel), "rel")
    if not src.is_cuda:
        raise ValueError("x_src must be a GPU tensor")
    if src.shape[1] < 1:
        raise ValueError("x_src needs at least one column")
    for name, t in (("x_dst", dst), ("rel", r)):
        if t.device != src.device or t.shape[1] != src.shape[1]:
            raise ValueError("%s must have the %d columns of x_src and live on %s" % (name, src.shape[1], src.device))
    if r.shape[0] < 1:
        raise ValueError("rel needs at least one row")
    if model in COMPLEX_MODELS and src.shape[1] % 2 != 0:
        raise ValueError("%s reads a row as [re | im]: F must be even (got %d)" % (model, src.shape[1]))
    row_ptr, col_ind = _block(csr_row_ptr, csr_col_ind, src.device, x_dst=dst)
    types = _index(edge_type, "edge_type", src.device)
    if types.shape[0] != col_ind.shape[0]:
        raise ValueError("edge_type has %d entries, csr_col_ind %d" % (types.shape[0], col_ind.shape[0]))
    return CscKgeScore.apply(src, dst, r, row_ptr, col_ind, types, MODELS[model], int(head == "src"))
