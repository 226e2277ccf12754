"""The GNN model surface of ``pylibwholegraph.torch.gnn_model`` (``set_framework``, ``create_gnn_layers``,
``create_sub_graph``, ``layer_forward``, ``HomoGNNModel``) for the ``cugraph`` framework route with GraphSAGE layers, on the
HIP aggregation op (``aggregation.py``), with GATv2 layers (model "gatv2": ``cugraphops.GATv2Conv`` on
``gatv2_aggregation.py``), with transformer layers (model "transformer": ``cugraphops.TransformerConv`` on
``transformer_aggregation.py``), with PNA layers (model "pna": ``cugraphops.PNAConv`` on ``pna_aggregation.py``, built by
``create_pna_layers``) and, for graphs with typed edges, with RGCN layers (model "rgcn": ``cugraphops.RGCNConv`` on
``rel_aggregation.py``, built by ``create_rgcn_layers``; the sampler delivers each block's edge types). The dgl / pyg / wg
routes and the model "gat" are not part of this build (the GAT layer itself is ``cugraphops.CuGraphGATConv``).

Flow of ``HomoGNNModel.forward`` (the reference's): sample ``layernum`` hops from the seed ids, gather the float32
features of the outermost frontier through ``WholeMemoryEmbeddingModule`` (so the embedding receives gradients), then one
layer per hop from the outermost block inwards, with relu and dropout between layers. With ``args.fuse_gather`` (an
extension, off by default) the outermost layer reads its rows from the embedding itself (``forward_from_table``) and the
feature gather is skipped: same logits and same embedding gradients, bit for bit."""
import torch
import torch.nn.functional as F

from .embedding import WholeMemoryEmbedding, WholeMemoryEmbeddingModule
from .graph_ops import add_csr_self_loop
from .graph_structure import GraphStructure
from .quantized import WholeMemoryQuantizedTensor

FRAMEWORKS = ("cugraph",)
framework_name = None
SAGEConv = None


def set_framework(framework: str):
    """Select the layer implementation: "cugraph" (CuGraphSAGEConv on the HIP aggregation op) is the one available."""
    global framework_name, SAGEConv
    if framework not in FRAMEWORKS:
        raise ValueError("framework %r is not available; available: %s" % (framework, ", ".join(FRAMEWORKS)))
    from .cugraphops.sage_conv import CuGraphSAGEConv
    framework_name = framework
    SAGEConv = CuGraphSAGEConv


def _require_framework():
    if framework_name is None:
        raise RuntimeError("call set_framework(...) first (available: %s)" % ", ".join(FRAMEWORKS))


def parse_max_neighbors(num_layer, neighbor_str):
    """"30,20" -> [30, 20]; a single number is used for every layer"""
    max_neighbors = [int(ns) for ns in str(neighbor_str).split(",")]
    if len(max_neighbors) not in (1, num_layer):
        raise ValueError("%d fan-outs given for %d layers" % (len(max_neighbors), num_layer))
    if len(max_neighbors) != num_layer:
        max_neighbors = max_neighbors * num_layer
    return max_neighbors


def create_gnn_layers(in_feat_dim, hidden_feat_dim, class_count, num_layer, num_head, model_type):
    _require_framework()
    if model_type == "gat":
        raise NotImplementedError("model 'gat' is not implemented on the cugraph route yet (only 'sage')")
    if model_type == "rgcn":
        raise ValueError("model 'rgcn' needs the number of relations: build its layers with create_rgcn_layers(in_feat_dim, "
                         "hidden_feat_dim, class_count, num_layer, num_relations, num_bases=None)")
    if model_type not in ("sage", "gatv2", "transformer"):
        raise ValueError("model %r is not available on the cugraph route (only 'sage', 'gatv2' and 'transformer')"
                         % (model_type,))
    gnn_layers = torch.nn.ModuleList()
    for i in range(num_layer):
        layer_output_dim = hidden_feat_dim // num_head if i != num_layer - 1 else class_count
        layer_input_dim = in_feat_dim if i == 0 else hidden_feat_dim
        if model_type == "gatv2":   # (the reference's flow for "gat": heads concatenated, averaged in the last layer)
            from .cugraphops.gatv2_conv import GATv2Conv
            gnn_layers.append(GATv2Conv(layer_input_dim, layer_output_dim, heads=num_head, concat=i != num_layer - 1))
        elif model_type == "transformer":   # (the same flow; the layer's root term is the target's own path)
            from .cugraphops.transformer_conv import TransformerConv
            gnn_layers.append(TransformerConv(layer_input_dim, layer_output_dim, heads=num_head,
                                              concat=i != num_layer - 1))
        else:
            gnn_layers.append(SAGEConv(layer_input_dim, layer_output_dim))
    return gnn_layers


def create_rgcn_layers(in_feat_dim, hidden_feat_dim, class_count, num_layer, num_relations, num_bases=None):
    """the layers of model "rgcn": RGCNConv(in -> hidden) ... RGCNConv(hidden -> class_count), each over `num_relations`
    relations (with `num_bases` basis matrices when given)"""
    _require_framework()
    from .cugraphops.rgcn_conv import RGCNConv
    gnn_layers = torch.nn.ModuleList()
    for i in range(num_layer):
        layer_output_dim = hidden_feat_dim if i != num_layer - 1 else class_count
        layer_input_dim = in_feat_dim if i == 0 else hidden_feat_dim
        gnn_layers.append(RGCNConv(layer_input_dim, layer_output_dim, num_relations, num_bases=num_bases))
    return gnn_layers


def create_pna_layers(in_feat_dim, hidden_feat_dim, class_count, num_layer, delta, aggregators=None, scalers=None):
    """the layers of model "pna": PNAConv(in -> hidden) ... PNAConv(hidden -> class_count), each with the degree scalers'
    `delta` (cugraphops.pna_delta of the training graph); `aggregators` / `scalers`: the layer's defaults when None"""
    _require_framework()
    from .cugraphops.pna_conv import PNAConv
    choice = {}
    if aggregators is not None:
        choice["aggregators"] = aggregators
    if scalers is not None:
        choice["scalers"] = scalers
    gnn_layers = torch.nn.ModuleList()
    for i in range(num_layer):
        layer_output_dim = hidden_feat_dim if i != num_layer - 1 else class_count
        layer_input_dim = in_feat_dim if i == 0 else hidden_feat_dim
        gnn_layers.append(PNAConv(layer_input_dim, layer_output_dim, delta=delta, **choice))
    return gnn_layers


def create_sub_graph(target_gid, target_gid_1, edge_data, csr_row_ptr, csr_col_ind, max_num_neighbors: int,
                     add_self_loop: bool):
    """[csr_row_ptr, csr_col_ind, max_num_neighbors] of one sampled block (the cugraph route's sub-graph)"""
    _require_framework()
    if add_self_loop:
        csr_row_ptr, csr_col_ind = add_csr_self_loop(csr_row_ptr, csr_col_ind)
        max_num_neighbors = max_num_neighbors + 1
    return [csr_row_ptr, csr_col_ind, max_num_neighbors]


def layer_forward(layer, x_feat, x_target_feat, sub_graph):
    _require_framework()
    return layer(x_feat, sub_graph[0], sub_graph[1], sub_graph[2])


class HomoGNNModel(torch.nn.Module):
    """Node classification model over a homogeneous graph: settings from an ``args`` namespace as the reference reads them
    (hiddensize, layernum, model, classnum, dropout, neighbors, inferencesample; heads for gat). Model "rgcn" (an
    extension) also reads num_relations, edge_type_name (an integer edge attribute registered with
    ``graph_structure.set_edge_attribute``: the relation of every graph edge) and, optionally, num_bases. Model "pna" (an
    extension) reads pna_delta (``cugraphops.pna_delta`` of the training graph) and, optionally, pna_aggregators and
    pna_scalers.
    ``node_embedding`` may also be a ``WholeMemoryQuantizedTensor`` (an extension: 8-bit row-quantized, frozen features):
    the features then come from its ``gather``, or with ``args.fuse_gather`` from layer 0's aggregation itself."""

    def __init__(self, graph_structure: GraphStructure, node_embedding, args):
        super().__init__()
        hidden_feat_dim = args.hiddensize
        self.graph_structure = graph_structure
        self.node_embedding = node_embedding
        self.num_layer = args.layernum
        self.hidden_feat_dim = args.hiddensize
        attention = args.model in ("gat", "gatv2")
        if args.model in ("gatv2", "transformer", "pna") and getattr(args, "fuse_gather", False):
            raise ValueError("fuse_gather reads layer 0's rows from the table: GraphSAGE only, not model %r" % args.model)
        num_head = args.heads if attention or args.model == "transformer" else 1
        assert hidden_feat_dim % num_head == 0
        in_feat_dim = self.node_embedding.shape[1]
        self.edge_type_name = None
        if args.model == "rgcn":
            if getattr(args, "fuse_gather", False):
                raise ValueError("fuse_gather reads layer 0's rows from the table: GraphSAGE only, not model 'rgcn'")
            if getattr(args, "num_relations", None) is None:
                raise ValueError("model 'rgcn' needs args.num_relations")
            if getattr(args, "edge_type_name", None) is None:
                raise ValueError("model 'rgcn' needs args.edge_type_name (an edge attribute of the graph structure)")
            self.edge_type_name = args.edge_type_name
            self.gnn_layers = create_rgcn_layers(in_feat_dim, hidden_feat_dim, args.classnum, args.layernum,
                                                 args.num_relations, getattr(args, "num_bases", None))
        elif args.model == "pna":
            if getattr(args, "pna_delta", None) is None:
                raise ValueError("model 'pna' needs args.pna_delta (cugraphops.pna_delta of the training graph)")
            self.gnn_layers = create_pna_layers(in_feat_dim, hidden_feat_dim, args.classnum, args.layernum, args.pna_delta,
                                                getattr(args, "pna_aggregators", None), getattr(args, "pna_scalers", None))
        else:
            self.gnn_layers = create_gnn_layers(in_feat_dim, hidden_feat_dim, args.classnum, args.layernum, num_head,
                                                args.model)
        self.mean_output = attention
        self.add_self_loop = attention
        if isinstance(self.node_embedding, WholeMemoryQuantizedTensor):   # (nothing to train: no embedding module)
            self.gather_fn = self.node_embedding.gather
        else:
            self.gather_fn = WholeMemoryEmbeddingModule(self.node_embedding)
        self.dropout = args.dropout
        self.max_neighbors = parse_max_neighbors(args.layernum, args.neighbors)
        self.max_inference_neighbors = parse_max_neighbors(args.layernum, getattr(args, "inferencesample", args.neighbors))
        self.fuse_gather = bool(getattr(args, "fuse_gather", False))

    def forward(self, ids):
        max_neighbors = self.max_neighbors if self.training else self.max_inference_neighbors
        ids = ids.to(self.graph_structure.csr_col_ind.dtype).cuda()
        edge_attrs = None
        if self.edge_type_name is not None:   # (model "rgcn": the relation of every sampled edge comes with its block)
            target_gids, edge_indice, csr_row_ptrs, csr_col_inds, edge_attrs = \
                self.graph_structure.multilayer_sample_with_edge_attributes(ids, max_neighbors, [self.edge_type_name])
        else:
            target_gids, edge_indice, csr_row_ptrs, csr_col_inds = \
                self.graph_structure.multilayer_sample_without_replacement(ids, max_neighbors)
        x_feat = None if self.fuse_gather else self.gather_fn(target_gids[0], force_dtype=torch.float32)
        for i in range(self.num_layer):
            sub_graph = create_sub_graph(target_gids[i], target_gids[i + 1], edge_indice[i], csr_row_ptrs[i],
                                         csr_col_inds[i], max_neighbors[self.num_layer - 1 - i], self.add_self_loop)
            if edge_attrs is not None:
                x_feat = self.gnn_layers[i](x_feat, sub_graph[0], sub_graph[1], sub_graph[2],
                                            edge_attrs[i][self.edge_type_name])
            elif x_feat is None:   # (layer 0 of the fused route: the rows come from the table, by id)
                x_feat = self.gnn_layers[0].forward_from_table(self.node_embedding, target_gids[0], sub_graph[0], sub_graph[1],
                                                               sub_graph[2], is_training=self.training)
            else:
                x_target_feat = x_feat[:target_gids[i + 1].numel()]
                x_feat = layer_forward(self.gnn_layers[i], x_feat, x_target_feat, sub_graph)
            if i != self.num_layer - 1:
                x_feat = F.relu(x_feat)
                x_feat = F.dropout(x_feat, self.dropout, training=self.training)
        return x_feat
