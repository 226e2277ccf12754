"""Subgraph-wise training (GraphSAINT, ShaDow-GNN, Cluster-GCN) on the ``cugraph`` route: a batch is a set of nodes and all
graph edges among them (``GraphStructure.induced_subgraph``, ``GraphStructure.saint_random_walk_subgraph``), and EVERY layer
runs on that one block with ``n_dst = n_src = n``, where ``HomoGNNModel`` runs layer i on the block of hop i.

``SubgraphGNNModel`` takes the settings ``HomoGNNModel`` reads (hiddensize, layernum, model, classnum, dropout; heads for the
attention models) and builds its layers with ``create_gnn_layers`` ("sage", "gatv2", "transformer"). Model "gat", which
``create_gnn_layers`` still refuses, is built here from ``cugraphops.CuGraphGATConv`` in the same flow: the heads concatenated,
averaged in the last layer. GraphSAINT's loss-normalisation coefficients are not part of this build."""
import torch
import torch.nn.functional as F

from .embedding import WholeMemoryEmbeddingModule
from .gnn_model import _require_framework, create_gnn_layers, create_sub_graph, layer_forward
from .graph_structure import GraphStructure
from .quantized import WholeMemoryQuantizedTensor


def _create_gat_layers(in_feat_dim, hidden_feat_dim, class_count, num_layer, num_head):
    _require_framework()
    from .cugraphops.gat_conv import CuGraphGATConv
    gnn_layers = torch.nn.ModuleList()
    for i in range(num_layer):
        layer_output_dim = hidden_feat_dim // num_head if i != num_layer - 1 else class_count
        layer_input_dim = in_feat_dim if i == 0 else hidden_feat_dim
        gnn_layers.append(CuGraphGATConv(layer_input_dim, layer_output_dim, heads=num_head, concat=i != num_layer - 1))
    return gnn_layers


class SubgraphGNNModel(torch.nn.Module):
    """Node classification on induced subgraphs. ``forward(nodes, offsets, col)`` takes what ``induced_subgraph(nodes)`` or
    ``saint_random_walk_subgraph`` returned, gathers the rows of ``nodes`` once (through ``WholeMemoryEmbeddingModule``, so the
    embedding receives gradients) and returns one row of logits per entry of ``nodes``."""

    def __init__(self, graph_structure: GraphStructure, node_embedding, args):
        super().__init__()
        self.graph_structure = graph_structure
        self.node_embedding = node_embedding
        self.num_layer = args.layernum
        self.hidden_feat_dim = args.hiddensize
        attention = args.model in ("gat", "gatv2")
        num_head = args.heads if attention or args.model == "transformer" else 1
        assert self.hidden_feat_dim % num_head == 0
        in_feat_dim = self.node_embedding.shape[1]
        if args.model == "gat":
            self.gnn_layers = _create_gat_layers(in_feat_dim, self.hidden_feat_dim, args.classnum, args.layernum, num_head)
        else:
            self.gnn_layers = create_gnn_layers(in_feat_dim, self.hidden_feat_dim, args.classnum, args.layernum, num_head,
                                                args.model)
        self.add_self_loop = attention      # (where HomoGNNModel adds them)
        if isinstance(self.node_embedding, WholeMemoryQuantizedTensor):   # (nothing to train: no embedding module)
            self.gather_fn = self.node_embedding.gather
        else:
            self.gather_fn = WholeMemoryEmbeddingModule(self.node_embedding)
        self.dropout = args.dropout

    def sub_graph(self, offsets, col):
        """[csr_row_ptr, csr_col_ind, max_num_neighbors] of the block as the layers take it (with self loops for the attention
        models); the same for every layer"""
        return create_sub_graph(None, None, None, offsets, col, 0, self.add_self_loop)

    def forward(self, nodes, offsets, col):
        x_feat = self.gather_fn(nodes, force_dtype=torch.float32)
        sub_graph = self.sub_graph(offsets, col)
        for i in range(self.num_layer):
            x_feat = layer_forward(self.gnn_layers[i], x_feat, x_feat, sub_graph)
            if i != self.num_layer - 1:
                x_feat = F.relu(x_feat)
                x_feat = F.dropout(x_feat, self.dropout, training=self.training)
        return x_feat
