"""Layers of the ``cugraph`` framework route (``gnn_model.set_framework("cugraph")``), on the HIP aggregation ops."""
from .edge_gat_conv import EdgeGATConv
from .gat_conv import CuGraphGATConv
from .gatv2_conv import GATv2Conv
from .pna_conv import PNAConv, pna_delta
from .rgcn_conv import RGCNConv
from .sage_conv import CuGraphSAGEConv
from .transformer_conv import TransformerConv
from .weighted_sage_conv import EdgeWeightedSAGEConv

__all__ = ["CuGraphSAGEConv", "CuGraphGATConv", "EdgeGATConv", "GATv2Conv", "RGCNConv", "TransformerConv", "PNAConv",
           "pna_delta", "EdgeWeightedSAGEConv"]
