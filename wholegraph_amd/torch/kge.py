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

from . import wholegraph_ops
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

    # ---- evaluation: the filtered rank of the true entity among all entities (``wholegraph_ops.rank_rows``) ----

    def rank_queries(self, anchor_rows: torch.Tensor, rel_rows: torch.Tensor) -> torch.Tensor:
        """[B, F]: the row q of a triple such that the model's score of entity row e on the corrupted side is ``rank_rows``'
        measure of (q, e). With a the anchor's row (the head under corrupt="tail", else the tail) and r the relation's:

        ===========  =======  ==================  ==========================================
        model        measure  corrupt="tail"      corrupt="head"
        ===========  =======  ==================  ==========================================
        distmult     dot      h * r               r * t
        transe_l1/2  l1 / l2  h + r               t - r
        complex      dot      h o r               conj(r) o t
        rotate       l2       h o r               conj(r) o t   (|h o r - t| = |h - conj(r) o t| needs |r| = 1,
                                                  which cat(cos, sin) of ``relation_rows`` has up to rounding)
        ===========  =======  ==================  ==========================================

        o is the complex product of header section 2u over rows read as [re | im]. l2 ranks by the squared distance."""
        a, r, tail = anchor_rows, rel_rows, self.corrupt == "tail"
        if self.model == "distmult":
            return a * r
        if self.model in ("transe_l1", "transe_l2"):
            return a + r if tail else a - r
        d = a.shape[1] // 2
        a_re, a_im, r_re, r_im = a[:, :d], a[:, d:], r[:, :d], r[:, d:]
        if tail:
            return torch.cat([a_re * r_re - a_im * r_im, a_re * r_im + a_im * r_re], dim=1)
        return torch.cat([r_re * a_re + r_im * a_im, r_re * a_im - r_im * a_re], dim=1)

    def known_neighbours(self, anchors: torch.Tensor):
        """(row_ptr int64 [B + 1], ids [M]): per anchor its distinct neighbours in graph_structure, ascending: the entities
        ``sample`` never draws as its negatives, and the filter block of ``rank`` and ``predict``"""
        g, n = self.graph_structure, anchors.shape[0]
        offset, nbr = wholegraph_ops.unweighted_sample_without_replacement(g.csr_row_ptr, g.csr_col_ind, anchors, -1)
        rows = torch.repeat_interleave(torch.arange(n, device=nbr.device), (offset[1:] - offset[:-1]).long())
        keys = torch.unique(rows * g.node_count + nbr.long())      # (sorted: by row, then id)
        row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=nbr.device)
        torch.cumsum(torch.bincount(torch.div(keys, g.node_count, rounding_mode="floor"), minlength=n), 0, out=row_ptr[1:])
        return row_ptr, (keys % g.node_count).to(anchors.dtype)

    def _table_queries(self, anchors: torch.Tensor, rels: torch.Tensor, filtered: bool, batch_size: int):
        """what ``rank`` and ``predict`` walk: per batch of anchors (slice, query rows, filter_row_ptr, filter_ids), then the
        entity table and the measure under which ``rank_queries``' rows score it"""
        table, rel = self.embedding.get_embedding_tensor(), self.relation_rows().detach()
        measure = {"distmult": "dot", "complex": "dot", "transe_l1": "l1"}.get(self.model, "l2")

        def batches():
            for s in range(0, anchors.shape[0], int(batch_size)):
                part = slice(s, s + int(batch_size))
                rows = self.embedding.gather(anchors[part], is_training=False, force_dtype=torch.float32)
                query = self.rank_queries(rows, rel.index_select(0, rels[part].long()))
                yield (part, query) + (self.known_neighbours(anchors[part]) if filtered else (None, None))
        return batches(), table, measure

    @torch.no_grad()
    def rank(self, triples: torch.Tensor, *, filtered: bool = True, batch_size: int = 1024):
        """(greater, equal), int64 [T] on the device: for every triple, how many entities on the side that ``corrupt`` names
        score above, and exactly, the true one (``rank_rows`` over the whole entity table; the true entity is left out).
        filtered: the known neighbours of the triple's anchor are left out too. Reads the table, changes nothing."""
        g = self.graph_structure
        if triples.dim() != 2 or triples.shape[1] != 3:
            raise ValueError("triples must be [T, 3] as (head, relation, tail) (got shape %s)" % (tuple(triples.shape),))
        heads, rels, tails = triples.to(g.csr_col_ind.dtype).cuda().t().contiguous().unbind(0)
        anchors, others = (heads, tails) if self.corrupt == "tail" else (tails, heads)
        batches, table, measure = self._table_queries(anchors, rels, filtered, batch_size)
        counts = torch.empty((2, anchors.shape[0]), dtype=torch.int64, device=anchors.device)
        for part, query, row_ptr, ids in batches:
            counts[0, part], counts[1, part] = wholegraph_ops.rank_rows(table, query, others[part], measure=measure,
                                                                        filter_row_ptr=row_ptr, filter_ids=ids)
        return counts[0], counts[1]

    @torch.no_grad()
    def predict(self, anchors: torch.Tensor, rels: torch.Tensor, k: int = 10, *, filtered: bool = True, batch_size: int = 1024):
        """(ids int64 [T, k], scores fp32 [T, k]) on the device: for every (anchor, relation) the k best entities on the side
        that ``corrupt`` names, best first, the lower id first among equal scores (``topk_rows`` over the whole entity table;
        k <= 64). The scores are ``rank``'s: the model's score, for the l2 models the negated SQUARED distance. filtered: the
        known neighbours of the anchor are left out. Where fewer than k entities remain the tail is -1 / NaN. Reads the
        table, changes nothing."""
        g = self.graph_structure
        if anchors.dim() != 1 or rels.shape != anchors.shape:
            raise ValueError("anchors and rels must be [T] (got %s and %s)" % (tuple(anchors.shape), tuple(rels.shape)))
        anchors, rels = anchors.to(g.csr_col_ind.dtype).cuda().contiguous(), rels.cuda()
        batches, table, measure = self._table_queries(anchors, rels, filtered, batch_size)
        ids = torch.empty((anchors.shape[0], int(k)), dtype=torch.int64, device=anchors.device)
        scores = torch.empty((anchors.shape[0], int(k)), dtype=torch.float32, device=anchors.device)
        for part, query, row_ptr, fids in batches:
            ids[part], scores[part] = wholegraph_ops.topk_rows(table, query, k, measure=measure, filter_row_ptr=row_ptr,
                                                               filter_ids=fids)
        return ids, scores

    @torch.no_grad()
    def test(self, triples: torch.Tensor, *, k=(1, 3, 10), filtered: bool = True, batch_size: int = 1024):
        """(mean_rank, mrr, {k: hits@k}) of the triples under the realistic rank 1 + greater + equal / 2 (PyG's
        ``KGEModel.test``, PyKEEN's "realistic")"""
        greater, equal = self.rank(triples, filtered=filtered, batch_size=batch_size)
        rank = 1.0 + greater.double() + equal.double() / 2.0
        if rank.shape[0] == 0:
            return float("nan"), float("nan"), {int(kk): float("nan") for kk in k}
        return float(rank.mean()), float((1.0 / rank).mean()), {int(kk): float((rank <= kk).double().mean()) for kk in k}
