"""GATv2 layer of the ``cugraph`` framework route: the constructor family and ``forward`` signature of ``CuGraphGATConv``
(cugraph-pyg's ``GATv2Conv`` on cugraph-ops' ``mha_gat_v2_n2n``) over this library's HIP ``mha_gat_v2_n2n`` op."""
import torch
from torch import Tensor
from torch.nn import Linear, Parameter

from ..gatv2_aggregation import mha_gat_v2_n2n


class GATv2Conv(torch.nn.Module):
    r"""The GATv2 operator of "How Attentive are Graph Attention Networks?" (Brody et al. 2022) on a sampled block.

    ``h_src = lin_src(x)`` ([n_src, heads * out_channels]) and ``h_dst = lin_dst(x[:n_dst])``; per target ``i`` and head
    ``k``, ``alpha_ij = softmax_j(att[k] . LeakyReLU(h_src_j + h_dst_i))`` and ``out_i = sum_j alpha_ij h_src_j``, the heads
    concatenated (``concat``) or averaged, plus ``bias``. ``att`` is ``[heads * out_channels]``, viewed as
    ``(heads, out_channels)``. With ``share_weights`` ``lin_dst`` is ``lin_src`` and ``h_dst = h_src[:n_dst]`` (autograd
    adds the two gradients). The block is given in CSC form: the neighbours of target ``i`` are
    ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]`` and the targets are the first ``len(csr_row_ptr) - 1`` rows of
    ``x`` (add self loops to let a target attend to itself).

    Edge features (``edge_dim``) are not built: the op has no edge term, and the layer takes none."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, bias: bool = True, share_weights: bool = False):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope
        self.share_weights = share_weights
        self.lin_src = Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src if share_weights else Linear(in_channels, heads * out_channels, bias=False)
        self.att = Parameter(torch.empty(heads * out_channels))
        if bias and concat:
            self.bias = Parameter(torch.empty(heads * out_channels))
        elif bias and not concat:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        torch.nn.init.xavier_normal_(self.lin_src.weight, gain=gain)
        if not self.share_weights:
            torch.nn.init.xavier_normal_(self.lin_dst.weight, gain=gain)
        torch.nn.init.xavier_normal_(self.att.data.view(self.heads, self.out_channels), gain=gain)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int) -> Tensor:
        # max_num_neighbors: a hint of the reference's fused kernel; the HIP op reads every target's degree from csr_row_ptr
        del max_num_neighbors
        n_dst = csr_row_ptr.shape[0] - 1
        h_src = self.lin_src(x)
        h_dst = h_src[:n_dst] if self.share_weights else self.lin_dst(x[:n_dst])
        out = mha_gat_v2_n2n(h_src, h_dst, self.att, csr_row_ptr, csr_col_ind, self.heads, self.negative_slope, self.concat)
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, heads=%d, share_weights=%s)" % (self.__class__.__name__, self.in_channels, self.out_channels,
                                                           self.heads, self.share_weights)
