"""The skip-gram block of wholegraph_amd/torch/skipgram.py restated with plain loops over walks, positions and offsets: the
centres are the entries >= 0 in row-major order; the edges of the centre at (i, t) are the positives walks[i, t + d] for
d = -W .. -1, 1 .. W inside the walk and >= 0 (label 1), then its negatives k = 0 .. K - 1 that are >= 0 (label 0)."""
import numpy as np


def skipgram_block_ref(walks, window, negatives=None):
    """-> (center_ids, row_ptr int32, ctx_ids, labels float32) from numpy arrays; ids in walks' dtype"""
    walks = np.asarray(walks)
    n, length = walks.shape[0], walks.shape[1] - 1
    centers, row_ptr, ctx, labels = [], [0], [], []
    for i in range(n):
        for t in range(length + 1):
            if walks[i, t] < 0:
                continue
            c = len(centers)
            centers.append(walks[i, t])
            for d in list(range(-window, 0)) + list(range(1, window + 1)):
                if 0 <= t + d <= length and walks[i, t + d] >= 0:
                    ctx.append(walks[i, t + d])
                    labels.append(1.0)
            if negatives is not None:
                for k in range(negatives.shape[1]):
                    if negatives[c, k] >= 0:
                        ctx.append(negatives[c, k])
                        labels.append(0.0)
            row_ptr.append(len(ctx))
    return (np.array(centers, walks.dtype), np.array(row_ptr, np.int32), np.array(ctx, walks.dtype),
            np.array(labels, np.float32))


def edge_count(walks, window, negatives=None):
    """E as the definition counts it: per centre, the live positions within `window` on its walk, and its live negatives"""
    walks = np.asarray(walks)
    live = walks >= 0
    total = 0
    for i in range(walks.shape[0]):
        for t in np.nonzero(live[i])[0]:
            lo, hi = max(0, t - window), min(walks.shape[1] - 1, t + window)
            total += int(live[i, lo:hi + 1].sum()) - 1
    if negatives is not None:
        total += int((np.asarray(negatives) >= 0).sum())
    return total
