"""Layers of the ``cugraph`` framework route (``gnn_model.set_framework("cugraph")``), on the HIP aggregation op."""
from .sage_conv import CuGraphSAGEConv

__all__ = ["CuGraphSAGEConv"]
