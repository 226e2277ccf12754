"""The sampled CSC block of tests/test_block_ops_capped_grid_gpu.py: the smallest one in which every kernel launch of a block
op has more work than one capped workgroup (WM_AGG_MAX_BLOCKS = 1 or 3) at every lane width, so that the second and later
trips of every grid-stride loop run (csrc/kernels/agg_common.cuh: blocks_for). A workgroup of 256 lanes holds 16, 8 or 4
lane groups (16, 32 or 64 lanes wide); under a cap of 3 a trip covers 48, 24 or 12 targets. With C = chunk_edges():

* n_dst = 301 targets, n_src = 1103 sources: neither is a multiple of 4, 8, 12, 16, 24 or 48, so the last trip of every loop
  over targets or sources is ragged at every lane width under both caps; 1103 sources are two node chunks of the attention
  ops' grad_att sums.
* about 35 edges per target, at least 20 C + 3 in all: more than 16 tiles of C sorted positions, so the chunk kernels of the
  per-source backward take a second trip even with 16 groups per workgroup.
* the degrees 0, 1, 8, 9, 17 and 65 (an empty target, one edge, around the batch of 8 rows, more than 16 and more than 64 lanes)
  on targets 0 .. 5 — the first four on the first trip at every lane width, all six on the first trip of the 16- and 32-lane
  kernels — and again on the last six targets, which every kernel reaches on a late, ragged trip.
* an early hub: source 0 has exactly C + 1 edges, one chunk boundary, its run at the start of the sorted positions.
* a late hub: source n_src - 1 has 2 C + 3 edges. Its run ends the sorted positions, so the tiles in which its chunks 1 and 2
  start have an index of at least 16: a second trip of for_chunk_pieces at every lane width.
* duplicate edges, and sources without edges on both sides of n_dst.

Built once per C and shared (read-only). tests/test_capped_block.py asserts all of this on the CPU."""
import functools

import numpy as np

N_DST, N_SRC = 301, 1103
BOUNDARY_DEGREES = (0, 1, 8, 9, 17, 65)
EARLY_HUB, LATE_HUB = 0, N_SRC - 1
NO_EDGES = (5, 150, N_DST + 7, N_SRC - 2)     # sources nobody reads: two targets, two that are none
DUPLICATE_IN = (4, 5, N_DST - 2, N_DST - 1)   # targets (degree 17 and 65, both times) whose first edge is there twice
MIN_TILES = 16                                # groups of the narrowest lane width in one workgroup


def min_edges(C):
    return 20 * C + 3


@functools.lru_cache(maxsize=None)
def capped_block(C):
    """(row_ptr [N_DST + 1] int32, col [E] int32), read-only"""
    rng = np.random.default_rng(20301)
    nb = len(BOUNDARY_DEGREES)
    deg = rng.integers(25, 46, N_DST)
    deg[:nb] = BOUNDARY_DEGREES
    deg[-nb:] = BOUNDARY_DEGREES
    free = np.arange(nb, N_DST - nb)
    while deg.sum() < min_edges(C):                      # (C = 512: the draw is already past it)
        deg[rng.choice(free, 50, replace=False)] += 1
    row_ptr = np.zeros(N_DST + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    E = int(row_ptr[-1])
    ordinary = np.setdiff1d(np.arange(N_SRC), (EARLY_HUB, LATE_HUB) + NO_EDGES)
    col = rng.choice(ordinary, E).astype(np.int32)
    for d in DUPLICATE_IN:
        col[row_ptr[d] + 1] = col[row_ptr[d]]
    keep = np.concatenate([[row_ptr[d], row_ptr[d] + 1] for d in DUPLICATE_IN])
    pos = rng.permutation(np.setdiff1d(np.arange(E), keep))[:3 * C + 4]
    col[pos[:C + 1]] = EARLY_HUB
    col[pos[C + 1:]] = LATE_HUB
    for a in (row_ptr, col):
        a.setflags(write=False)
    return row_ptr, col
