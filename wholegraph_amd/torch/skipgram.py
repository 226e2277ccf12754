"""The skip-gram block of a batch of walks: every (centre, context) pair within a window of a walk, and the negatives drawn
for the centres, as one CSC block whose targets are the centre positions — what ``edge_dot_n2n`` scores and ``Node2Vec``
trains on. Plain torch ops on whatever device the walks live on (CPU tensors too); no loop over walks or positions.

``walks [n, L + 1]`` (int32 or int64) is what ``GraphStructure.random_walk`` / ``node2vec_walk`` return: a negative entry
is "no node" (the walk ops write -1 behind a walk's end). The centres are the entries >= 0 in row-major order. The edges of
the centre at ``(i, t)`` are, in this order, the positives ``walks[i, t + d]`` for ``d = -W .. -1, 1 .. W`` with
``0 <= t + d <= L`` and an entry >= 0 (label 1; a context equal to the centre is kept), then the centre's negatives
``k = 0 .. K - 1`` that are >= 0 (label 0)."""
import torch

_MAX_EDGES = 1 << 31


def _checked_walks(walks: torch.Tensor) -> torch.Tensor:
    if walks.dim() != 2 or walks.shape[1] < 1:
        raise ValueError("walks must be [n, L + 1] (got shape %s)" % (tuple(walks.shape),))
    if walks.dtype not in (torch.int32, torch.int64):
        raise TypeError("walks must be int32 or int64 (got %s)" % walks.dtype)
    return walks


def centers_of(walks: torch.Tensor) -> torch.Tensor:
    """center_ids [Tc]: the entries of walks that are >= 0, in row-major order — what the negatives are drawn for"""
    walks = _checked_walks(walks)
    return walks[walks >= 0]


def _edge_count_bound(n_positions: int, reach: int, num_negatives: int) -> int:
    """the most edges n_positions centres can have: 2 * reach positives and num_negatives negatives each"""
    return int(n_positions) * (2 * int(reach) + int(num_negatives))


def _exact_edge_count(walks: torch.Tensor, reach: int, negatives) -> int:
    """E by counting, without building the block: the pairs d apart on one walk count for +d and for -d"""
    live = walks >= 0
    total = torch.zeros((), dtype=torch.int64, device=walks.device)
    for d in range(1, reach + 1):   # (over the window, not over walks or positions)
        total += 2 * (live[:, d:] & live[:, :-d]).sum()
    if negatives is not None:
        total += (negatives >= 0).sum()
    return int(total)


def _refuse_too_many(n_edges: int):
    if n_edges >= _MAX_EDGES:
        raise ValueError("the block would have %d edges: row_ptr is int32, so fewer than 2^31" % n_edges)


def skipgram_block(walks: torch.Tensor, window: int, negatives=None):
    """-> (center_ids [Tc], row_ptr int32 [Tc + 1], ctx_ids [E], labels float32 [E]); center_ids and ctx_ids are global ids in
    walks' dtype. negatives: None or [Tc, K], row c the negatives of centre c (``centers_of(walks)[c]``); negative entries
    are "none". Fewer than 2^31 edges, else ValueError."""
    walks = _checked_walks(walks)
    window = int(window)
    if window < 1:
        raise ValueError("window must be >= 1 (got %d)" % window)
    n, length = walks.shape[0], walks.shape[1] - 1
    reach = min(window, length)   # (no two positions of a walk are further apart than its length)
    dev = walks.device
    live = walks >= 0
    center_ids = walks[live]
    n_centers = center_ids.shape[0]
    num_neg = 0
    if negatives is not None:
        if negatives.dim() != 2 or negatives.shape[0] != n_centers:
            raise ValueError("negatives must be [%d, K], a row per centre (got shape %s)" % (n_centers, tuple(negatives.shape)))
        if negatives.dtype not in (torch.int32, torch.int64) or negatives.device != dev:
            raise TypeError("negatives must be int32 or int64 on %s (got %s on %s)" % (dev, negatives.dtype, negatives.device))
        num_neg = negatives.shape[1]
    # the candidates are materialised below: a batch that could reach 2^31 edges is counted first
    if _edge_count_bound(walks.numel(), reach, num_neg) >= _MAX_EDGES:
        _refuse_too_many(_exact_edge_count(walks, reach, negatives))
    offsets = torch.cat([torch.arange(-reach, 0, device=dev), torch.arange(1, reach + 1, device=dev)])
    pos = torch.arange(length + 1, device=dev)[:, None] + offsets[None, :]            # [L + 1, 2 * reach]
    inside = (pos >= 0) & (pos <= length)
    cand = torch.where(inside[None], walks[:, pos.clamp(0, length)], walks.new_full((), -1))   # [n, L + 1, 2 * reach]
    cand = cand[live]                                                                  # [Tc, 2 * reach]
    label_row = torch.ones(2 * reach, dtype=torch.float32, device=dev)
    if negatives is not None:
        cand = torch.cat([cand, negatives.to(walks.dtype)], dim=1)
        label_row = torch.cat([label_row, torch.zeros(num_neg, dtype=torch.float32, device=dev)])
    valid = cand >= 0
    row_ptr = torch.zeros(n_centers + 1, dtype=torch.int64, device=dev)
    torch.cumsum(valid.sum(1), 0, out=row_ptr[1:])
    ctx_ids = cand[valid]
    _refuse_too_many(ctx_ids.shape[0])
    labels = label_row[None, :].expand(n_centers, -1)[valid]
    return center_ids, row_ptr.to(torch.int32), ctx_ids, labels
