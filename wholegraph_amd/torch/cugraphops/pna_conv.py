"""Principal Neighbourhood Aggregation layer: the aggregator / scaler family of PyG's ``PNAConv`` and the ``forward``
signature of ``CuGraphSAGEConv``, over this library's HIP ``agg_concat_pna`` op."""
import math
from typing import Optional

import torch
from torch import Tensor
from torch.nn import Linear

from ..pna_aggregation import aggregator_mask, aggregator_names, agg_concat_pna

SCALERS = ("identity", "amplification", "attenuation")


def pna_delta(csr_row_ptr: Tensor) -> float:
    """delta of the degree scalers: the mean of log(deg + 1) over the targets of a row pointer tensor [n + 1] (the training
    graph's, for the layer's constructor)"""
    if csr_row_ptr.dim() != 1 or csr_row_ptr.shape[0] < 2:
        raise ValueError("csr_row_ptr must be 1-D with at least two entries")
    deg = (csr_row_ptr[1:] - csr_row_ptr[:-1]).to(torch.float64)
    return float(torch.log(deg + 1).mean())


class PNAConv(torch.nn.Module):
    r"""The operator of "Principal Neighbourhood Aggregation for Graph Nets" (Corso et al. 2020) on a sampled block.

    With ``project``, first ``h = relu(pre_lin(x))`` (else ``h = x``). ``A = agg_concat_pna(h, ...)`` holds one block of
    ``in_channels`` columns per aggregator (in the order sum, mean, min, max, std) and the target's own row. Each scaler
    multiplies the aggregator blocks by a scalar per target of degree ``deg``: ``identity`` by 1, ``amplification`` by
    ``log(deg + 1) / delta``, ``attenuation`` by ``delta / log(deg + 1)`` (0 for ``deg = 0``). The scaled blocks are
    concatenated scaler by scaler, the own row is appended with ``root_weight``, and ``out = lin(...)`` maps the
    ``(len(aggregators) * len(scalers) + root_weight) * in_channels`` columns to ``out_channels``. ``delta`` is the mean of
    ``log(deg + 1)`` over the training graph (``pna_delta``); it is required with a scaler other than ``identity``. The block
    is given in CSC form: the neighbours of target ``i`` are ``x[csr_col_ind[csr_row_ptr[i]:csr_row_ptr[i + 1]]]`` and the
    targets are the first ``len(csr_row_ptr) - 1`` rows of ``x``. The scaling is plain torch; the op's kernels know nothing of
    it. ``PNAConv(..., aggregators=["max"], scalers=["identity"])`` is GraphSAGE with the max aggregator.

    Differences from PyG's ``PNAConv``: one tower; no per-edge pre-MLP on ``cat(x_i, x_j)`` (the projection acts per node, so
    the aggregation reads each neighbour row once); no ``edge_dim``; the ``var`` aggregator and the ``linear`` /
    ``inverse_linear`` scalers are not built; a target without edges gets 0 in the std block where PyG gives ``sqrt(eps)``."""

    def __init__(self, in_channels: int, out_channels: int, aggregators=("mean", "min", "max", "std"),
                 scalers=("identity", "amplification", "attenuation"), delta: Optional[float] = None, project: bool = False,
                 root_weight: bool = True, bias: bool = True):
        super().__init__()
        self.aggregators = aggregator_names(aggregator_mask(aggregators))   # (slot order; ValueError for a bad list)
        scalers = [scalers] if isinstance(scalers, str) else list(scalers)
        if not scalers:
            raise ValueError("scalers must name at least one of %s" % ", ".join(SCALERS))
        for i, name in enumerate(scalers):
            if name not in SCALERS:
                raise ValueError("unknown scaler %r (one of %s)" % (name, ", ".join(SCALERS)))
            if name in scalers[:i]:
                raise ValueError("scaler %r is listed twice" % (name,))
        if any(name != "identity" for name in scalers):
            if delta is None:
                raise ValueError("delta (the mean of log(deg + 1) over the training graph: pna_delta) is required with the "
                                 "scalers %s" % ", ".join(scalers))
            if not (delta > 0 and math.isfinite(delta)):
                raise ValueError("delta must be positive and finite (got %r)" % (delta,))
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.scalers = scalers
        self.delta = None if delta is None else float(delta)
        self.root_weight = root_weight
        self.pre_lin = Linear(in_channels, in_channels) if project else None
        blocks = len(self.aggregators) * len(scalers) + (1 if root_weight else 0)
        self.lin = Linear(blocks * in_channels, out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        if self.pre_lin is not None:
            self.pre_lin.reset_parameters()
        self.lin.reset_parameters()

    def forward(self, x: Tensor, csr_row_ptr: Tensor, csr_col_ind: Tensor, max_num_neighbors: int) -> Tensor:
        # max_num_neighbors: a hint of the reference's fused kernel; the HIP op reads every target's degree from csr_row_ptr
        del max_num_neighbors
        h = torch.relu(self.pre_lin(x)) if self.pre_lin is not None else x
        agg = agg_concat_pna(h, csr_row_ptr, csr_col_ind, self.aggregators)
        width = len(self.aggregators) * self.in_channels
        stats, own = agg[:, :width], agg[:, width:]
        blocks = []
        if self.scalers != ["identity"]:
            logd = torch.log((csr_row_ptr[1:] - csr_row_ptr[:-1]).to(agg.dtype) + 1).unsqueeze(1)
        for name in self.scalers:
            if name == "identity":
                blocks.append(stats)
            elif name == "amplification":
                blocks.append(stats * (logd / self.delta))
            else:   # attenuation: 0 for a target without edges
                blocks.append(stats * torch.where(logd > 0, self.delta / logd, torch.zeros_like(logd)))
        if self.root_weight:
            blocks.append(own)
        return self.lin(torch.cat(blocks, dim=1) if len(blocks) > 1 else blocks[0])

    def __repr__(self) -> str:
        return "%s(%d, %d, aggregators=%s, scalers=%s)" % (self.__class__.__name__, self.in_channels, self.out_channels,
                                                          self.aggregators, self.scalers)
