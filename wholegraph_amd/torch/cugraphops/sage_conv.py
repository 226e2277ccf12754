"""GraphSAGE layer of the ``cugraph`` route: ``pylibwholegraph.torch.cugraphops.sage_conv.CuGraphSAGEConv`` (same
constructor, parameters and ``forward`` signature) over this library's HIP ``agg_concat`` op."""
import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn import Linear

from ..aggregation import aggr_code, agg_concat
from ..gather_aggregation import gather_agg_concat


class CuGraphSAGEConv(torch.nn.Module):
    r"""GraphSAGE ("Inductive Representation Learning on Large Graphs", Hamilton et al. 2017) on a sampled block.

    ``out = lin(cat(aggr_{j in N(i)} x_j, x_i))`` with ``root_weight`` (else ``lin(aggr x_j)``); ``project`` first maps
    ``x`` through ``relu(pre_lin(x))``; ``normalize`` L2-normalises the output rows. The block is given in CSC form:
    the neighbours of target ``i`` are ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]`` and the targets are the
    first ``len(csr_row_ptr) - 1`` rows of ``x``.

    Mixed precision needs no argument: the aggregation runs in the dtype of its input (float32, float16 or bfloat16; with
    16-bit rows the sums are still taken in fp32 and rounded once). So the layer works after ``.half()`` / ``.bfloat16()``
    on input of that dtype, and under ``torch.autocast``, where a layer fed by another layer's ``Linear`` output
    aggregates 16-bit rows."""

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

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int) -> Tensor:
        # max_num_neighbors: a hint of the reference's fused kernel; the HIP op reads every target's degree from csr_row_ptr
        del max_num_neighbors
        if self.project:
            x = self.pre_lin(x).relu()
        return self._after_aggregation(agg_concat(x, csr_row_ptr, csr_col_ind, self.aggr))

    def forward_from_table(self, source, node_ids: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int,
                           is_training: bool = False) -> Tensor:
        """``forward`` whose ``x`` is ``source[node_ids]`` (a ``WholeMemoryEmbedding`` or ``WholeMemoryTensor``, rows widened
        to float32, or a ``WholeMemoryQuantizedTensor``, rows dequantized), read by the aggregation itself
        (``gather_agg_concat``): the first layer of a model without the gathered feature matrix. Same result as
        ``forward(source.gather(node_ids, force_dtype=torch.float32), ...)``, bit for bit. ``is_training``: hand the row
        gradients to the embedding's optimizer, as ``WholeMemoryEmbeddingModule`` does (a quantized table is frozen)."""
        del max_num_neighbors
        if self.project:
            raise ValueError("forward_from_table needs project=False: pre_lin must see the rows before they are aggregated")
        return self._after_aggregation(gather_agg_concat(source, node_ids, csr_row_ptr, csr_col_ind, self.aggr,
                                                         is_training=is_training))

    def _after_aggregation(self, out: Tensor) -> Tensor:
        if self.root_weight:
            out = self.lin(out)
        else:
            out = self.lin(out[:, :self.in_channels])
        if self.normalize:
            out = F.normalize(out, p=2.0, dim=-1)
        return out

    def __repr__(self) -> str:
        return "%s(%d, %d, aggr=%s)" % (self.__class__.__name__, self.in_channels, self.out_channels, self.aggr)
