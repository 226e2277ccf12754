"""GAT layer of the ``cugraph`` route: ``pylibwholegraph.torch.cugraphops.gat_conv.CuGraphGATConv`` (same constructor,
parameters and ``forward`` signature) over this library's HIP ``mha_gat_n2n`` op."""
import torch
from torch import Tensor
from torch.nn import Linear, Parameter

from ..gat_aggregation import mha_gat_n2n


class CuGraphGATConv(torch.nn.Module):
    r"""The graph attention operator of "Graph Attention Networks" (Velickovic et al. 2018) on a sampled block.

    ``h = lin(x)`` ([n_src, heads * out_channels]); per target ``i`` and head ``k``,
    ``alpha_ij = softmax_j(LeakyReLU(att[0, k] . h_j + att[1, k] . h_i))`` and ``out_i = sum_j alpha_ij h_j``, the heads
    concatenated (``concat``) or averaged, plus ``bias``. ``att`` is ``[2 * heads * out_channels]``, viewed as
    ``(2, heads, out_channels)``: half 0 the source (neighbour) side, half 1 the target side. The block is given in CSC
    form: the neighbours of target ``i`` are ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]`` and the targets are the
    first ``len(csr_row_ptr) - 1`` rows of ``x`` (add self loops to let a target attend to itself)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, bias: bool = True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope
        self.lin = Linear(in_channels, heads * out_channels, bias=False)
        self.att = Parameter(torch.empty(2 * heads * out_channels))
        if bias and concat:
            self.bias = Parameter(torch.empty(heads * out_channels))
        elif bias and not concat:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        torch.nn.init.xavier_normal_(self.lin.weight, gain=gain)
        att = self.att.data.view(2, self.heads, self.out_channels)
        torch.nn.init.xavier_normal_(att[0, :, :], gain=gain)
        torch.nn.init.xavier_normal_(att[1, :, :], gain=gain)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int) -> Tensor:
        # max_num_neighbors: a hint of the reference's fused kernel; the HIP op reads every target's degree from csr_row_ptr
        del max_num_neighbors
        out = mha_gat_n2n(self.lin(x), self.att, csr_row_ptr, csr_col_ind, self.heads, self.negative_slope, self.concat)
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, heads=%d)" % (self.__class__.__name__, self.in_channels, self.out_channels, self.heads)
