"""Layers of the ``cugraph`` framework route (``gnn_model.set_framework("cugraph")``), on the HIP aggregation ops."""
from .gat_conv import CuGraphGATConv
from .sage_conv import CuGraphSAGEConv

__all__ = ["CuGraphSAGEConv", "CuGraphGATConv"]
