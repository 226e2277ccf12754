"""Transformer layer of the ``cugraph`` framework route: the constructor family of cugraph-pyg's ``TransformerConv`` (on
cugraph-ops' ``mha_simple_n2n``) and the ``forward`` signature of ``CuGraphGATConv``, over this library's HIP
``mha_simple_n2n`` op."""
import torch
from torch import Tensor
from torch.nn import Linear

from ..transformer_aggregation import mha_simple_n2n


class TransformerConv(torch.nn.Module):
    r"""The graph transformer operator of "Masked Label Prediction: Unified Message Passing Model for Semi-Supervised
    Classification" (Shi et al. 2021) on a sampled block.

    ``query = lin_query(x[:n_dst])``, ``key = lin_key(x)`` and ``value = lin_value(x)`` (each to ``heads * out_channels``
    columns, with bias); per target ``i`` and head ``k``, ``alpha_ij = softmax_j(query_i . key_j / sqrt(out_channels))`` and
    ``out_i = sum_j alpha_ij value_j``, the heads concatenated (``concat``) or averaged. With ``root_weight`` the skip term
    ``x_r = lin_skip(x[:n_dst])`` is added: ``out + x_r``, or with ``beta`` the gated
    ``b * x_r + (1 - b) * out``, ``b = sigmoid(lin_beta([out, x_r, out - x_r]))``. The block is given in CSC form: the
    neighbours of target ``i`` are ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]`` and the targets are the first
    ``len(csr_row_ptr) - 1`` rows of ``x`` (the root term is the target's own path: no self loops are needed).

    Edge features (``edge_dim``) and dropout of the attention weights are not built: the op has no edge term and keeps every
    weight, and the layer takes neither."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True, beta: bool = False,
                 bias: bool = True, root_weight: bool = True):
        super().__init__()
        if beta and not root_weight:
            raise ValueError("beta gates the root term: it needs root_weight=True")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.concat = concat
        self.beta = beta
        self.root_weight = root_weight
        self.lin_key = Linear(in_channels, heads * out_channels)
        self.lin_query = Linear(in_channels, heads * out_channels)
        self.lin_value = Linear(in_channels, heads * out_channels)
        width = heads * out_channels if concat else out_channels
        self.lin_skip = Linear(in_channels, width, bias=bias) if root_weight else None
        self.lin_beta = Linear(3 * width, 1, bias=False) if beta else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int) -> Tensor:
        # max_num_neighbors: a hint of the reference's fused kernel; the HIP op reads every target's degree from csr_row_ptr
        del max_num_neighbors
        n_dst = csr_row_ptr.shape[0] - 1
        x_dst = x[:n_dst]
        out = mha_simple_n2n(self.lin_key(x), self.lin_query(x_dst), self.lin_value(x), csr_row_ptr, csr_col_ind, self.heads,
                             concat=self.concat, norm_by_dim=True)
        if self.root_weight:
            x_r = self.lin_skip(x_dst)
            if self.lin_beta is not None:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)))
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, heads=%d)" % (self.__class__.__name__, self.in_channels, self.out_channels, self.heads)
