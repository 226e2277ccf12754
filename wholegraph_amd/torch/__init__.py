"""wholegraph_amd.torch — the ``pylibwholegraph.torch`` surface of the embedding path on MI355X.

Same names and signatures as reference ``python/pylibwholegraph/pylibwholegraph/torch/__init__.py:14-78`` for
communicators, initialisation, WholeMemory tensors, embeddings / optimizers / cache policies, the gather / scatter
functors, neighbour sampling and GraphStructure, and for the GNN model surface of the ``cugraph`` framework route
(``set_framework``, ``create_gnn_layers``, ``create_sub_graph``, ``HomoGNNModel``; the GraphSAGE and GAT layers in
``cugraphops``, on the HIP ops of ``aggregation`` and ``gat_aggregation``; and, beyond the reference, the edge-weighted
GraphSAGE layer ``cugraphops.EdgeWeightedSAGEConv`` on ``weighted_aggregation``, the GAT layer with edge features
``cugraphops.EdgeGATConv`` on ``edge_gat_aggregation``, the GATv2 layer ``cugraphops.GATv2Conv`` on ``gatv2_aggregation``
(model name "gatv2"), the RGCN layer ``cugraphops.RGCNConv`` on ``rel_aggregation`` (model name "rgcn"), the transformer
layer ``cugraphops.TransformerConv`` on ``transformer_aggregation`` (model name "transformer"), the PNA layer
``cugraphops.PNAConv`` on ``pna_aggregation`` (sum / mean / min / max / std in one pass; model name "pna"), and
``gather_aggregation``, layer 0's aggregation straight from a
WholeMemory table, and ``quantized``, 8-bit row-quantized tables whose gather dequantizes the rows it reads; and
``edge_dot.edge_dot_n2n``, the score of an edge as the dot product of its endpoint rows, with ``skipgram.skipgram_block`` and
the ``node2vec.Node2Vec`` model that train embeddings on the walks and negatives of ``GraphStructure``; and
``saint.SubgraphGNNModel``, the layers above on the induced subgraphs of ``GraphStructure.induced_subgraph`` and
``GraphStructure.saint_random_walk_subgraph``: subgraph-wise training; and ``temporal.TimeEncoder`` and
``temporal.TemporalGNNModel``, ``EdgeGATConv`` layers over the temporal trees of ``GraphStructure.multilayer_temporal_sample``,
whose edges never lie in their centre's future). GAT in
``HomoGNNModel``, the dgl / pyg / wg routes, data loaders, launch helpers and option parsers of the reference are outside this build's scope.
"""
from . import comm, embedding, graph_ops, graph_structure, initialize, tensor, utils, wholegraph_ops, wholememory_ops
from . import aggregation, cugraphops, edge_gat_aggregation, gat_aggregation, gather_aggregation, gnn_model
from . import gatv2_aggregation, pna_aggregation, quantized, rel_aggregation, transformer_aggregation, weighted_aggregation
from . import edge_dot, node2vec, saint, skipgram, temporal

_PUBLIC = {
    comm: ("WholeMemoryCommunicator create_group_communicator destroy_communicator get_global_communicator "
           "get_local_node_communicator get_local_device_communicator split_communicator get_local_mnnvl_communicator"),
    embedding: ("WholeMemoryOptimizer create_wholememory_optimizer destroy_wholememory_optimizer WholeMemoryCachePolicy "
                "create_builtin_cache_policy create_wholememory_cache_policy destroy_wholememory_cache_policy "
                "WholeMemoryEmbedding create_embedding create_embedding_from_filelist destroy_embedding "
                "WholeMemoryEmbeddingModule"),
    initialize: "init init_torch_env init_torch_env_and_create_wm_comm finalize",
    tensor: ("WholeMemoryTensor create_wholememory_tensor create_wholememory_tensor_from_filelist "
             "destroy_wholememory_tensor"),
    utils: "get_part_file_name get_part_file_list wholememory_dtype_to_torch_dtype torch_dtype_to_wholememory_dtype",
    wholememory_ops: "wholememory_gather_forward_functor wholememory_scatter_functor",
    graph_structure: "GraphStructure",
    gnn_model: "set_framework create_gnn_layers create_rgcn_layers create_pna_layers create_sub_graph HomoGNNModel",
    gather_aggregation: "gather_agg_concat",
    pna_aggregation: "agg_concat_pna",
    edge_dot: "edge_dot_n2n",
    skipgram: "skipgram_block centers_of",
    node2vec: "Node2Vec",
    saint: "SubgraphGNNModel",
    temporal: "TimeEncoder TemporalGNNModel",
    quantized: ("WholeMemoryQuantizedTensor create_quantized_tensor quantized_row_bytes quantize_rows "
                "dequantize_rows"),
}
__all__ = ["graph_ops", "wholegraph_ops", "aggregation", "cugraphops", "gat_aggregation", "gnn_model", "weighted_aggregation",
           "gather_aggregation", "edge_gat_aggregation", "gatv2_aggregation", "rel_aggregation", "quantized",
           "transformer_aggregation", "pna_aggregation", "edge_dot", "skipgram", "node2vec", "saint", "temporal"]
for _module, _names in _PUBLIC.items():
    for _name in _names.split():
        globals()[_name] = getattr(_module, _name)
        __all__.append(_name)
del _module, _names, _name
