"""GAT layer with edge features in the attention logit (PyG's ``GATConv(edge_dim=...)``, cugraph-ops'
``mha_gat_n2n(..., edge_feat=...)``): ``CuGraphGATConv`` plus ``lin_edge`` and a third slice of ``att``, over this library's HIP
``mha_gat_n2n_edge`` op. Beyond the reference, whose GAT layer takes no edge input."""
import torch
from torch import Tensor
from torch.nn import Linear, Parameter

from ..edge_gat_aggregation import mha_gat_n2n_edge


class EdgeGATConv(torch.nn.Module):
    r"""The graph attention operator on a sampled block whose edges carry attributes.

    ``h = lin(x)`` ([n_src, heads * out_channels]) and ``g = lin_edge(edge_attr)`` ([E, heads * out_channels]); per target
    ``i``, head ``k`` and edge ``e = (j -> i)``,
    ``alpha_e = softmax_e(LeakyReLU(att[0, k] . h_j + att[1, k] . h_i + att[2, k] . g_e))`` and ``out_i = sum_e alpha_e h_j``,
    the heads concatenated (``concat``) or averaged, plus ``bias``: the edge attributes steer the attention and are not
    aggregated themselves. ``att`` is ``[3 * heads * out_channels]``, viewed as ``(3, heads, out_channels)``: source, target
    and edge side. The block is given in CSC form as for ``CuGraphGATConv``; row ``e`` of ``edge_attr`` ([E, edge_dim], or
    [E] for a scalar attribute, what ``GraphStructure.multilayer_sample_with_edge_attributes`` returns for one) belongs to
    edge position ``e`` of ``csr_col_ind``.

    The layer takes the block as sampled: it adds no self loops, and self loops added by the caller have no sampled
    attribute — give them a row of ``edge_attr`` of your choosing, or leave them out."""

    def __init__(self, in_channels: int, out_channels: int, edge_dim: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, bias: bool = True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.edge_dim = edge_dim
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope
        self.lin = Linear(in_channels, heads * out_channels, bias=False)
        self.lin_edge = Linear(edge_dim, heads * out_channels, bias=False)
        self.att = Parameter(torch.empty(3 * heads * out_channels))
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
        torch.nn.init.xavier_normal_(self.lin_edge.weight, gain=gain)
        att = self.att.data.view(3, self.heads, self.out_channels)
        for half in range(3):
            torch.nn.init.xavier_normal_(att[half, :, :], gain=gain)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, edge_attr: Tensor,
                max_num_neighbors: int = None) -> Tensor:
        # max_num_neighbors: a hint of the reference's fused kernel; the HIP op reads every target's degree from csr_row_ptr
        del max_num_neighbors
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.unsqueeze(1)
        if edge_attr.dim() != 2 or edge_attr.shape[1] != self.edge_dim:
            raise ValueError("edge_attr must be [E, %d] (got shape %s)" % (self.edge_dim, tuple(edge_attr.shape)))
        if not edge_attr.is_floating_point():
            edge_attr = edge_attr.to(self.lin_edge.weight.dtype)
        out = mha_gat_n2n_edge(self.lin(x), self.att, self.lin_edge(edge_attr), csr_row_ptr, csr_col_ind, self.heads,
                               self.negative_slope, self.concat)
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, edge_dim=%d, heads=%d)" % (self.__class__.__name__, self.in_channels, self.out_channels,
                                                      self.edge_dim, self.heads)
