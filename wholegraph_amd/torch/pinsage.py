"""PinSAGE (Ying et al., KDD 2018) on the ``cugraph`` route: the neighbours of a node are the nodes that short random walks
with restart visit most often (``GraphStructure.multilayer_pinsage_sample``), and a layer pools them by importance, the visit
counts normalised per target. ``PinSAGEModel`` is a stack of ``cugraphops.EdgeWeightedSAGEConv(aggr="sum")`` fed those
weights: they sum to 1 per target, which turns the sum into PinSAGE's weighted mean; the layer's root term is the target's
own row, which is why arrivals at the seed are not counted by the sampler."""
import torch
import torch.nn.functional as F

from .embedding import WholeMemoryEmbeddingModule
from .gnn_model import _require_framework, parse_max_neighbors
from .graph_structure import GraphStructure
from .quantized import WholeMemoryQuantizedTensor


class PinSAGEModel(torch.nn.Module):
    """Node classification over importance neighbourhoods. ``forward(seeds)`` samples the blocks, gathers the rows of the
    outermost frontier (through ``WholeMemoryEmbeddingModule``, so the embedding receives gradients) and returns one row of
    logits per seed. It reads hiddensize, layernum, classnum, dropout and neighbors as ``HomoGNNModel`` does, and num_walks,
    walk_length and restart_prob (default 0.5) for the walks."""

    def __init__(self, graph_structure: GraphStructure, node_embedding, args):
        super().__init__()
        _require_framework()
        from .cugraphops.weighted_sage_conv import EdgeWeightedSAGEConv
        self.graph_structure = graph_structure
        self.node_embedding = node_embedding
        self.num_layer = args.layernum
        self.hidden_feat_dim = args.hiddensize
        in_feat_dim = self.node_embedding.shape[1]
        self.gnn_layers = torch.nn.ModuleList()
        for i in range(self.num_layer):
            last = i == self.num_layer - 1
            self.gnn_layers.append(EdgeWeightedSAGEConv(in_feat_dim if i == 0 else self.hidden_feat_dim,
                                                        args.classnum if last else self.hidden_feat_dim, aggr="sum"))
        if isinstance(self.node_embedding, WholeMemoryQuantizedTensor):   # (nothing to train: no embedding module)
            self.gather_fn = self.node_embedding.gather
        else:
            self.gather_fn = WholeMemoryEmbeddingModule(self.node_embedding)
        self.dropout = args.dropout
        self.max_neighbors = parse_max_neighbors(args.layernum, args.neighbors)
        self.num_walks, self.walk_length = args.num_walks, args.walk_length
        self.restart_prob = getattr(args, "restart_prob", 0.5)

    def sample(self, seeds, random_seeds=None):
        """the importance blocks of the seeds: what ``multilayer_pinsage_sample`` returns"""
        seeds = seeds.to(self.graph_structure.csr_col_ind.dtype).cuda()
        return self.graph_structure.multilayer_pinsage_sample(
            seeds, self.max_neighbors, num_walks=self.num_walks, walk_length=self.walk_length, restart_prob=self.restart_prob,
            random_seeds=random_seeds)

    def forward(self, seeds, random_seeds=None):
        target_gids, _, csr_row_ptrs, csr_col_inds, importances = self.sample(seeds, random_seeds)
        x_feat = self.gather_fn(target_gids[0], force_dtype=torch.float32)
        for i in range(self.num_layer):
            x_feat = self.gnn_layers[i](x_feat, csr_row_ptrs[i], csr_col_inds[i], 0, importances[i])
            if i != self.num_layer - 1:
                x_feat = F.relu(x_feat)
                x_feat = F.dropout(x_feat, self.dropout, training=self.training)
        return x_feat
