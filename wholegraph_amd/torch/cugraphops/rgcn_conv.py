"""Relational GCN layer: the constructor family of PyG's ``RGCNConv`` (cugraph-pyg's layer on cugraph-ops'
``agg_hg_basis_n2n_post``) over this library's HIP ``agg_concat_rel`` op (``forward`` takes the edge types of the block as
a fifth argument)."""
from typing import Optional

import torch
from torch import Tensor
from torch.nn import Parameter

from ..aggregation import aggr_code
from ..rel_aggregation import agg_concat_rel


class RGCNConv(torch.nn.Module):
    r"""The relational graph convolution of "Modeling Relational Data with Graph Convolutional Networks" (Schlichtkrull et
    al. 2018) on a sampled block: ``out_i = sum_r W_r aggr_{j in N_r(i)} x_j + root x_i + bias``. The block is given in CSC
    form: the neighbours of target ``i`` are ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]``, the relation of the edge
    at position ``e`` of ``csr_col_ind`` is ``edge_type[e]`` (in ``[0, num_relations)``; an edge with any other value
    contributes nothing), and the targets are the first ``len(csr_row_ptr) - 1`` rows of ``x``.

    The layer is a linear map of the op's output ``agg = agg_concat_rel(x, ...)`` (``[n_dst, (R + 1) * F]``):
    ``agg[:, :R * F] @ W.view(R * F, O) + agg[:, R * F:] @ root + bias``. Parameters: ``weight`` ``[R, F, O]``, or
    ``[num_bases, F, O]`` with ``comp`` ``[R, num_bases]`` when ``num_bases`` is given (basis decomposition:
    ``W = comp @ weight``, formed in torch on every call); ``root`` ``[F, O]`` with ``root_weight``; ``bias`` ``[O]``.
    Folding the basis coefficients into the aggregation kernel (cugraph-ops' ``agg_hg_basis_n2n_post``, which aggregates
    into ``num_bases`` slots) is out of scope: the op always aggregates per relation.

    ``aggr="mean"`` is the mean over the edges of each relation (the paper's ``c_{i,r} = |N_r(i)|``, PyG's default).
    cugraph-ops' mean over the target's TOTAL degree is ``aggr="sum"`` with the result divided by the degree.

    The aggregation is fp32: under ``torch.autocast`` a 16-bit input is widened on the way into the op; outside autocast a
    16-bit ``x`` is a ``TypeError``."""

    def __init__(self, in_channels: int, out_channels: int, num_relations: int, num_bases: Optional[int] = None,
                 aggr: str = "mean", root_weight: bool = True, bias: bool = True):
        super().__init__()
        if aggr not in ("mean", "sum", "min", "max"):
            raise ValueError("Aggregation function must be either 'mean', 'sum', 'min' or 'max' (got %r)" % (aggr,))
        aggr_code(aggr)   # max / min: NotImplementedError here rather than at the first forward
        if num_relations < 1:
            raise ValueError("num_relations must be >= 1 (got %d)" % num_relations)
        if num_bases is not None and num_bases < 1:
            raise ValueError("num_bases must be >= 1 or None (got %d)" % num_bases)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_relations = num_relations
        self.num_bases = num_bases
        self.aggr = aggr
        self.root_weight = root_weight
        self.weight = Parameter(torch.empty(num_relations if num_bases is None else num_bases, in_channels, out_channels))
        if num_bases is not None:
            self.comp = Parameter(torch.empty(num_relations, num_bases))
        else:
            self.register_parameter("comp", None)
        if root_weight:
            self.root = Parameter(torch.empty(in_channels, out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        torch.nn.init.xavier_uniform_(self.weight, gain=gain)
        if self.comp is not None:
            torch.nn.init.xavier_uniform_(self.comp, gain=gain)
        if self.root is not None:
            torch.nn.init.xavier_uniform_(self.root, gain=gain)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int,
                edge_type: Tensor) -> Tensor:
        # max_num_neighbors: kept for call-site symmetry with CuGraphSAGEConv; the HIP op reads degrees from csr_row_ptr
        del max_num_neighbors
        agg = agg_concat_rel(x, csr_row_ptr, csr_col_ind, edge_type, self.num_relations, self.aggr)
        rf = self.num_relations * self.in_channels
        weight = self.weight
        if self.comp is not None:
            weight = (self.comp @ weight.view(self.num_bases, -1)).view(self.num_relations, self.in_channels, -1)
        out = agg[:, :rf] @ weight.view(rf, self.out_channels)
        if self.root is not None:
            out = out + agg[:, rf:] @ self.root
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, num_relations=%d, num_bases=%s, aggr=%s)" % (
            self.__class__.__name__, self.in_channels, self.out_channels, self.num_relations, self.num_bases, self.aggr)
