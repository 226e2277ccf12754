"""GraphSAGE layer with a weight per edge: the constructor, parameters and initialisation of ``CuGraphSAGEConv``, over this
library's HIP ``agg_concat_weighted`` op (``forward`` takes the edge weights of the block as a fifth argument)."""
import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn import Linear

from ..aggregation import aggr_code
from ..weighted_aggregation import agg_concat_weighted


class EdgeWeightedSAGEConv(torch.nn.Module):
    r"""``out = lin(cat(aggr_{j in N(i)} w_ij x_j, x_i))`` with ``root_weight`` (else ``lin(aggr w_ij x_j)``) on a sampled
    block in CSC form: the neighbours of target ``i`` are ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]``, the
    weight of the edge at position ``e`` of ``csr_col_ind`` is ``edge_weight[e]``, and the targets are the first
    ``len(csr_row_ptr) - 1`` rows of ``x``. ``aggr="mean"`` divides the weighted sum by the target's degree (DGL's
    edge-weight convention). ``project`` first maps ``x`` through ``relu(pre_lin(x))``; ``normalize`` L2-normalises the
    output rows. Gradients flow into ``x`` and into ``edge_weight`` (GCN-style normalisation constants, importance
    corrections of a weighted sample and learnable edge gates are all just a tensor of ``E`` floats here).

    The aggregation is fp32: under ``torch.autocast`` a 16-bit input is widened on the way into the op; outside autocast a
    16-bit ``x`` is a ``TypeError``."""

    def __init__(self, in_channels: int, out_channels: int, aggr: str = "mean", normalize: bool = False,
                 root_weight: bool = True, project: bool = False, bias: bool = True):
        super().__init__()
        if aggr not in ("mean", "sum", "min", "max"):
            raise ValueError("Aggregation function must be either 'mean', 'sum', 'min' or 'max' (got %r)" % (aggr,))
        aggr_code(aggr)   # max / min: NotImplementedError here rather than at the first forward
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.aggr = aggr
        self.normalize = normalize
        self.root_weight = root_weight
        self.project = project
        if self.project:
            self.pre_lin = Linear(in_channels, in_channels, bias=True)
        self.lin = Linear((2 if root_weight else 1) * in_channels, out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        torch.nn.init.xavier_uniform_(self.lin.weight, gain=gain)
        if self.project:
            torch.nn.init.xavier_uniform_(self.pre_lin.weight, gain=gain)

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int,
                edge_weight: Tensor) -> Tensor:
        # max_num_neighbors: kept for call-site symmetry with CuGraphSAGEConv; the HIP op reads degrees from csr_row_ptr
        del max_num_neighbors
        if self.project:
            x = self.pre_lin(x).relu()
        out = agg_concat_weighted(x, csr_row_ptr, csr_col_ind, edge_weight, self.aggr)
        if self.root_weight:
            out = self.lin(out)
        else:
            out = self.lin(out[:, :self.in_channels])
        if self.normalize:
            out = F.normalize(out, p=2.0, dim=-1)
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, aggr=%s)" % (self.__class__.__name__, self.in_channels, self.out_channels, self.aggr)
