"""Temporal graph learning on an interaction graph (TGAT, TGN without its memory module; PyG's ``NeighborLoader`` with
``time_attr``) on the ``cugraph`` route: a seed is a node WITH a time, its neighbourhood is sampled by
``GraphStructure.multilayer_temporal_sample`` — disjoint trees, no edge from a centre's future — and every layer is an
``EdgeGATConv`` whose edge feature is the time encoding of ``t_centre - t_edge``.

``TimeEncoder`` is TGAT's functional time encoding. ``TemporalGNNModel`` takes the settings ``HomoGNNModel`` reads (hiddensize,
layernum, classnum, dropout, heads, neighbors, inferencesample) and, optionally, time_dim (default: hiddensize),
temporal_strategy ("uniform" / "last"), temporal_inclusive, time_window and temporal_propagate ("seed" / "edge")."""
import torch
import torch.nn.functional as F

from .embedding import WholeMemoryEmbeddingModule
from .gnn_model import _require_framework, parse_max_neighbors
from .graph_structure import GraphStructure
from .quantized import WholeMemoryQuantizedTensor


class TimeEncoder(torch.nn.Module):
    """TGAT's time encoding ``cos(dt * w + b)`` -> [..., dim], ``w`` initialised to ``10 ** -linspace(0, 9, dim)`` and ``b`` to
    0, both trained; ``dt`` is taken as fp32."""

    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim
        self.lin = torch.nn.Linear(1, dim)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.lin.weight.copy_((10.0 ** -torch.linspace(0, 9, self.dim, dtype=torch.float64)).to(torch.float32).reshape(self.dim, 1))
            self.lin.bias.zero_()

    def forward(self, dt: torch.Tensor) -> torch.Tensor:
        return torch.cos(self.lin(dt.to(torch.float32).unsqueeze(-1)))


class TemporalGNNModel(torch.nn.Module):
    """Node classification at a point in time: ``forward(seeds, seed_times)`` samples the temporal trees of the seeds, gathers
    the rows of the outermost frontier once (through ``WholeMemoryEmbeddingModule``, so the embedding receives gradients) and
    returns one row of logits per seed. Layer i runs ``EdgeGATConv`` on the block of hop i with the edge feature
    ``TimeEncoder(target_time - edge_time)`` and adds a linear map of the target's own row, since a tree block has no self
    loops and a centre without an eligible neighbour aggregates nothing. `time_name` names the int64 edge attribute that
    holds the edge times."""

    def __init__(self, graph_structure: GraphStructure, node_embedding, args, time_name: str):
        super().__init__()
        _require_framework()
        from .cugraphops.edge_gat_conv import EdgeGATConv
        self.graph_structure = graph_structure
        self.node_embedding = node_embedding
        self.time_name = time_name
        self.num_layer = args.layernum
        self.hidden_feat_dim = args.hiddensize
        num_head = getattr(args, "heads", 1)
        assert self.hidden_feat_dim % num_head == 0
        time_dim = getattr(args, "time_dim", None) or self.hidden_feat_dim
        in_feat_dim = self.node_embedding.shape[1]
        self.time_encoder = TimeEncoder(time_dim)
        self.gnn_layers, self.self_layers = torch.nn.ModuleList(), torch.nn.ModuleList()
        for i in range(self.num_layer):
            last = i == self.num_layer - 1
            layer_input_dim = in_feat_dim if i == 0 else self.hidden_feat_dim
            layer_output_dim = args.classnum if last else self.hidden_feat_dim // num_head
            self.gnn_layers.append(EdgeGATConv(layer_input_dim, layer_output_dim, time_dim, heads=num_head, concat=not last))
            self.self_layers.append(torch.nn.Linear(layer_input_dim, args.classnum if last else self.hidden_feat_dim, bias=False))
        if isinstance(self.node_embedding, WholeMemoryQuantizedTensor):   # (nothing to train: no embedding module)
            self.gather_fn = self.node_embedding.gather
        else:
            self.gather_fn = WholeMemoryEmbeddingModule(self.node_embedding)
        self.dropout = args.dropout
        self.max_neighbors = parse_max_neighbors(args.layernum, args.neighbors)
        self.max_inference_neighbors = parse_max_neighbors(args.layernum, getattr(args, "inferencesample", args.neighbors))
        self.strategy = getattr(args, "temporal_strategy", "uniform")
        self.inclusive = bool(getattr(args, "temporal_inclusive", True))
        self.time_window = getattr(args, "time_window", None)
        self.propagate = getattr(args, "temporal_propagate", "seed")

    def sample(self, seeds, seed_times, random_seeds=None):
        """the temporal trees of the seeds: what ``multilayer_temporal_sample`` returns with the edge times as attribute"""
        max_neighbors = self.max_neighbors if self.training else self.max_inference_neighbors
        seeds = seeds.to(self.graph_structure.csr_col_ind.dtype).cuda()
        seed_times = seed_times.to(torch.int64).cuda()
        return self.graph_structure.multilayer_temporal_sample(
            seeds, seed_times, max_neighbors, self.time_name, strategy=self.strategy, inclusive=self.inclusive,
            time_window=self.time_window, propagate=self.propagate, random_seeds=random_seeds, edge_attr_names=[self.time_name])

    def forward(self, seeds, seed_times, random_seeds=None):
        target_gids, target_times, edge_indice, csr_row_ptrs, csr_col_inds, _, edge_attrs = self.sample(seeds, seed_times,
                                                                                                       random_seeds)
        x_feat = self.gather_fn(target_gids[0], force_dtype=torch.float32)
        for i in range(self.num_layer):
            n_target = target_gids[i + 1].numel()
            centre_time = target_times[i + 1][edge_indice[i][1].long()]
            edge_feat = self.time_encoder(centre_time - edge_attrs[i][self.time_name])
            x_target = x_feat[:n_target]
            x_feat = self.gnn_layers[i](x_feat, csr_row_ptrs[i], csr_col_inds[i], edge_feat) + self.self_layers[i](x_target)
            if i != self.num_layer - 1:
                x_feat = F.relu(x_feat)
                x_feat = F.dropout(x_feat, self.dropout, training=self.training)
        return x_feat
