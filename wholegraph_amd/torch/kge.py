"""Knowledge-graph embeddings (DistMult, TransE, ComplEx, RotatE) trained on filtered negatives: ``kge_block`` turns a batch
of triples and their negatives into the CSC block ``kge_score_n2n`` scores, and ``KGEModel`` draws the negatives over a
``GraphStructure``, gathers the entity rows of a WholeMemory embedding and holds the relation table. Sampling is seeded,
every sum of the op and of the sparse optimizer's duplicate fold has one order, so a run from the same seeds ends with the
same tables bit for bit.

``kge_block`` is plain torch ops on whatever device the triples live on (CPU tensors too). Target c of the block is positive
triple c, anchored at ``heads[c]``; its edges are, in this order, the true ``tails[c]`` (label 1) and the negatives of row c
that are >= 0 (label 0); every edge of the row carries ``rels[c]``."""
import math
from typing import NamedTuple, Union

import torch
import torch.nn.functional as F

from .embedding import EmbeddingLookupFn, WholeMemoryEmbedding
from .graph_ops import append_unique
from .graph_structure import GraphStructure
from .kge_score import COMPLEX_MODELS, MODELS, kge_score_n2n


def kge_block(heads: torch.Tensor, rels: torch.Tensor, tails: torch.Tensor, negatives=None):
    """-> (row_ptr int32 [T + 1], ctx_ids [E], edge_type int32 [E], labels float32 [E]); ctx_ids are global ids in tails'
    dtype. heads, rels, tails: [T] integer tensors; negatives: None or [T, K], row c the corrupted tails of triple c, negative
    entries are "none"."""
    if not (heads.dim() == rels.dim() == tails.dim() == 1 and heads.shape == rels.shape == tails.shape):
        raise ValueError("heads, rels and tails must be 1-D of one length (got %s, %s, %s)" % (
            tuple(heads.shape), tuple(rels.shape), tuple(tails.shape)))
    for name, t in (("heads", heads), ("rels", rels), ("tails", tails)):
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s must be int32 or int64 (got %s)" % (name, t.dtype))
    n, dev = tails.shape[0], tails.device
    cand = tails[:, None]
    label_row = torch.ones(1, dtype=torch.float32, device=dev)
    if negatives is not None:
        if negatives.dim() != 2 or negatives.shape[0] != n:
            raise ValueError("negatives must be [%d, K], a row per triple (got shape %s)" % (n, tuple(negatives.shape)))
        if negatives.dtype not in (torch.int32, torch.int64) or negatives.device != dev:
            raise TypeError("negatives must be int32 or int64 on %s (got %s on %s)" % (dev, negatives.dtype, negatives.device))
        cand = torch.cat([cand, negatives.to(tails.dtype)], dim=1)
        label_row = torch.cat([label_row, torch.zeros(negatives.shape[1], dtype=torch.float32, device=dev)])
    valid = cand >= 0
    valid[:, 0] = True   # (the true tail is an edge whatever its id: a bad id is the caller's to find)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(valid.sum(1), 0, out=row_ptr[1:])
    if int(row_ptr[-1]) >= 1 << 31:
        raise ValueError("the block would have %d edges: row_ptr is int32, so fewer than 2^31" % int(row_ptr[-1]))
    width = cand.shape[1]
    edge_type = rels.to(device=dev, dtype=torch.int32)[:, None].expand(-1, width)[valid]
    labels = label_row[None, :].expand(n, -1)[valid]
    return row_ptr.to(torch.int32), cand[valid], edge_type, labels


class KGEBatch(NamedTuple):
    """what ``KGEModel.sample`` returns: the block of ``kge_block`` with its contexts made unique"""
    anchor_ids: torch.Tensor   # [T] global ids: target c of the block (the heads; the tails with corrupt="head")
    row_ptr: torch.Tensor      # int32 [T + 1]
    ctx_ids: torch.Tensor      # [E] global ids: per triple its true other end, then its negatives
    edge_type: torch.Tensor    # int32 [E]
    labels: torch.Tensor       # float32 [E]: 1 a positive, 0 a negative
    unique_ctx: torch.Tensor   # [n_src] global ids: source row j of the block
    col_ind: torch.Tensor      # int32 [E]: unique_ctx[col_ind] == ctx_ids


class KGEModel(torch.nn.Module):
    """A knowledge-graph embedding model scored by ``kge_score_n2n``.

    graph_structure: the CSR graph of the known triples in WholeMemory (what the negatives are filtered against);
    embedding: the entity table, [n_nodes, F] fp32, trained through its WholeMemory optimizer (``EmbeddingLookupFn``);
    num_relations R; model one of "distmult", "transe_l1", "transe_l2", "complex", "rotate"; num_negatives K per triple;
    margin: added to every score ahead of the logistic loss (the gamma of the distance models). The relation table is a dense
    ``torch.nn.Parameter`` for a torch optimizer: [R, F], or for "rotate" the phases [R, F / 2], from which
    ``cat(cos, sin)`` is formed in torch so that autograd carries the phase gradient. corrupt: "tail" (the anchor of a
    triple is its head and the negatives replace the tail) or "head" (the anchor is the tail, the op runs with head="src").
    The negatives of a triple are non-neighbours of its anchor in graph_structure."""

    def __init__(self, graph_structure: GraphStructure, embedding: WholeMemoryEmbedding, num_relations: int, *,
                 model: str = "distmult", num_negatives: int = 4, margin: float = 0.0, corrupt: str = "tail",
                 negative_mode: str = "uniform", col_sorted: bool = False):
        super().__init__()
        if model not in MODELS:
            raise ValueError("model must be one of %s (got %r)" % (", ".join(MODELS), model))
        if corrupt not in ("tail", "head"):
            raise ValueError("corrupt must be 'tail' or 'head' (got %r)" % (corrupt,))
        if int(num_relations) < 1 or int(num_negatives) < 0:
            raise ValueError("num_relations >= 1 and num_negatives >= 0 (got %r, %r)" % (num_relations, num_negatives))
        dim = int(embedding.get_embedding_tensor().shape[1])
        if model in COMPLEX_MODELS and dim % 2 != 0:
            raise ValueError("%s reads a row as [re | im]: the embedding width must be even (got %d)" % (model, dim))
        self.graph_structure = graph_structure
        self.embedding = embedding
        self.model, self.corrupt = model, corrupt
        self.num_relations, self.num_negatives, self.margin = int(num_relations), int(num_negatives), float(margin)
        self.negative_mode, self.col_sorted = negative_mode, bool(col_sorted)
        if model == "rotate":
            init = (torch.rand(self.num_relations, dim // 2) * 2.0 - 1.0) * math.pi
        else:
            init = torch.randn(self.num_relations, dim) * 0.1 + (1.0 if model in ("distmult", "complex") else 0.0)
            if model == "complex":
                init[:, dim // 2:] -= 1.0   # (re near 1, im near 0: the identity relation)
        self.relation = torch.nn.Parameter(init.cuda())

    def relation_rows(self) -> torch.Tensor:
        """[R, F]: the table the op reads"""
        if self.model == "rotate":
            return torch.cat([torch.cos(self.relation), torch.sin(self.relation)], dim=1)
        return self.relation

    def sample(self, triples: torch.Tensor, random_seed: Union[int, None] = None) -> KGEBatch:
        """triples [T, 3] as (head, relation, tail): negatives for the anchors, the block and its unique contexts"""
        g = self.graph_structure
        if triples.dim() != 2 or triples.shape[1] != 3:
            raise ValueError("triples must be [T, 3] as (head, relation, tail) (got shape %s)" % (tuple(triples.shape),))
        heads, rels, tails = triples.to(g.csr_col_ind.dtype).cuda().t().contiguous().unbind(0)   # (each unit-stride)
        anchors, others = (heads, tails) if self.corrupt == "tail" else (tails, heads)
        negatives = None
        if self.num_negatives > 0 and anchors.shape[0] > 0:
            negatives = g.negative_sample(anchors, self.num_negatives, mode=self.negative_mode, random_seed=random_seed,
                                          col_sorted=self.col_sorted)
        row_ptr, ctx_ids, edge_type, labels = kge_block(anchors, rels, others, negatives)
        if ctx_ids.shape[0] > 0:
            unique_ctx, col_ind = append_unique(ctx_ids[:0], ctx_ids, need_neighbor_raw_to_unique=True)
        else:
            unique_ctx, col_ind = ctx_ids, torch.zeros(0, dtype=torch.int32, device=ctx_ids.device)
        return KGEBatch(anchors, row_ptr, ctx_ids, edge_type, labels, unique_ctx, col_ind)

    def _rows(self, ids: torch.Tensor) -> torch.Tensor:
        table = self.embedding
        return EmbeddingLookupFn.apply(ids, table.dummy_input, table, self.training, torch.float32)

    def score_edges(self, x_src, x_dst, rel, batch: KGEBatch) -> torch.Tensor:
        return kge_score_n2n(x_src, x_dst, rel, batch.row_ptr, batch.col_ind, batch.edge_type, model=self.model,
                             head="dst" if self.corrupt == "tail" else "src")

    def scores(self, batch: KGEBatch) -> torch.Tensor:
        """[E]: the score of every edge of the block. A row per triple on the anchor side: an entity that anchors several
        triples is gathered once for each, and the sparse optimizer adds their gradients in order."""
        return self.score_edges(self._rows(batch.unique_ctx), self._rows(batch.anchor_ids), self.relation_rows(), batch)

    def loss(self, batch: KGEBatch) -> torch.Tensor:
        """-mean(logsigmoid(margin + s[positives])) - mean(logsigmoid(-(margin + s[negatives]))); a side without edges
        contributes 0"""
        s = self.scores(batch) + self.margin
        pos = batch.labels > 0.5
        sides = [F.logsigmoid(t).mean() for t in (s[pos], -s[~pos]) if t.shape[0] > 0]
        if not sides:
            return s.sum()   # (no edge: 0, with the graph attached)
        return -sides[0] if len(sides) == 1 else -sides[0] - sides[1]

    def forward(self, triples: torch.Tensor, random_seed: Union[int, None] = None) -> torch.Tensor:
        return self.loss(self.sample(triples, random_seed))
