"""DeepWalk / node2vec embeddings trained on the fused walks and negatives: ``Node2Vec`` samples a batch of walks over a
``GraphStructure``, draws negatives for the centres, builds the skip-gram block (``skipgram.py``) and scores its edges with
``edge_dot_n2n`` on rows of a WholeMemory embedding. The loss is PyG's ``Node2Vec`` loss. Sampling is seeded, every sum of
the op and of the sparse optimizer's duplicate fold has one order, so a run from the same seeds ends with the same table bit
for bit."""
from typing import NamedTuple, Optional, Union

import torch
import torch.nn.functional as F

from .edge_dot import edge_dot_n2n
from .embedding import EmbeddingLookupFn, WholeMemoryEmbedding
from .graph_ops import append_unique
from .graph_structure import GraphStructure
from .skipgram import centers_of, skipgram_block


class SkipGramBatch(NamedTuple):
    """what ``Node2Vec.sample`` returns: the block of ``skipgram_block`` with its contexts made unique"""
    walks: torch.Tensor        # [n, walk_length + 1], -1 behind a walk's end
    center_ids: torch.Tensor   # [Tc] global ids: target c of the block
    row_ptr: torch.Tensor      # int32 [Tc + 1]
    ctx_ids: torch.Tensor      # [E] global ids
    labels: torch.Tensor       # float32 [E]: 1 a positive, 0 a negative
    unique_ctx: torch.Tensor   # [n_src] global ids: source row j of the block
    col_ind: torch.Tensor      # int32 [E]: unique_ctx[col_ind] == ctx_ids


class Node2Vec(torch.nn.Module):
    """Skip-gram with negative sampling over random walks (p == q == 1: DeepWalk) or node2vec (p, q) walks.

    graph_structure: the CSR graph in WholeMemory; embedding: the table of centre rows, [n_nodes, F] fp32, trained through
    its WholeMemory optimizer (``EmbeddingLookupFn``); context_embedding: a second table for the context rows (word2vec's
    "output" vectors), else both sides read ``embedding``. walk_length steps a walk, window W, num_negatives K per centre
    position (0: none), weight_name an edge attribute that weighs the steps, negative_mode "uniform" or "degree", col_sorted
    the caller's promise that the rows of csr_col_ind are ascending."""

    def __init__(self, graph_structure: GraphStructure, embedding: WholeMemoryEmbedding, *, walk_length: int, window: int,
                 num_negatives: int, p: float = 1.0, q: float = 1.0, weight_name: Optional[str] = None,
                 negative_mode: str = "uniform", col_sorted: bool = False,
                 context_embedding: Optional[WholeMemoryEmbedding] = None):
        super().__init__()
        if int(walk_length) < 1 or int(window) < 1 or int(num_negatives) < 0:
            raise ValueError("walk_length >= 1, window >= 1 and num_negatives >= 0 (got %r, %r, %r)" % (
                walk_length, window, num_negatives))
        self.graph_structure = graph_structure
        self.embedding = embedding
        self.context_embedding = context_embedding
        self.walk_length, self.window, self.num_negatives = int(walk_length), int(window), int(num_negatives)
        self.p, self.q = float(p), float(q)
        self.weight_name = weight_name
        self.negative_mode = negative_mode
        self.col_sorted = bool(col_sorted)

    def sample(self, start_nodes: torch.Tensor, random_seed: Union[int, None] = None) -> SkipGramBatch:
        """walks from start_nodes, negatives for their centres, the skip-gram block and its unique contexts. The negatives'
        seed is derived from random_seed (the two ops would otherwise read the same random streams)."""
        g = self.graph_structure
        start_nodes = start_nodes.to(g.csr_col_ind.dtype).cuda()
        if self.p == 1.0 and self.q == 1.0:
            walks = g.random_walk(start_nodes, self.walk_length, weight_name=self.weight_name, random_seed=random_seed)
        else:
            walks = g.node2vec_walk(start_nodes, self.walk_length, self.p, self.q, weight_name=self.weight_name,
                                    random_seed=random_seed, col_sorted=self.col_sorted)
        centers = centers_of(walks)
        negatives = None
        if self.num_negatives > 0 and centers.shape[0] > 0:
            neg_seed = None if random_seed is None else (int(random_seed) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
            negatives = g.negative_sample(centers, self.num_negatives, mode=self.negative_mode, random_seed=neg_seed,
                                          col_sorted=self.col_sorted)
        center_ids, row_ptr, ctx_ids, labels = skipgram_block(walks, self.window, negatives)
        if ctx_ids.shape[0] > 0:
            unique_ctx, col_ind = append_unique(ctx_ids[:0], ctx_ids, need_neighbor_raw_to_unique=True)   # (only ids >= 0)
        else:
            unique_ctx, col_ind = ctx_ids, torch.zeros(0, dtype=torch.int32, device=ctx_ids.device)
        return SkipGramBatch(walks, center_ids, row_ptr, ctx_ids, labels, unique_ctx, col_ind)

    def _rows(self, table: WholeMemoryEmbedding, ids: torch.Tensor) -> torch.Tensor:
        return EmbeddingLookupFn.apply(ids, table.dummy_input, table, self.training, torch.float32)

    def scores(self, batch: SkipGramBatch) -> torch.Tensor:
        """[E]: the dot product of every edge's centre row and context row. A row per centre position: a node that is the
        centre of several positions is gathered once for each, and the sparse optimizer adds their gradients in order."""
        x_dst = self._rows(self.embedding, batch.center_ids)
        x_src = self._rows(self.context_embedding if self.context_embedding is not None else self.embedding, batch.unique_ctx)
        return edge_dot_n2n(x_src, x_dst, batch.row_ptr, batch.col_ind)

    def loss(self, batch: SkipGramBatch) -> torch.Tensor:
        """-mean(logsigmoid(s[positives])) - mean(logsigmoid(-s[negatives])); a side without edges contributes 0"""
        s = self.scores(batch)
        pos = batch.labels > 0.5
        sides = [F.logsigmoid(t).mean() for t in (s[pos], -s[~pos]) if t.shape[0] > 0]
        if not sides:
            return s.sum()   # (no edge: 0, with the graph attached)
        return -sides[0] if len(sides) == 1 else -sides[0] - sides[1]

    def forward(self, start_nodes: torch.Tensor, random_seed: Union[int, None] = None) -> torch.Tensor:
        return self.loss(self.sample(start_nodes, random_seed))

    def embed(self, ids: torch.Tensor) -> torch.Tensor:
        """the rows of `ids`: a plain gather, no gradient"""
        return self.embedding.gather(ids.to(self.graph_structure.csr_col_ind.dtype).cuda(), force_dtype=torch.float32)
