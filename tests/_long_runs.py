"""A sampled CSC block whose per-source backward walks more than one batch of partial rows (csrc/kernels/agg_common.cuh,
add_partials): the kernels load kAggBatch = 8 partial rows back to back, and a source of n chunks has n - 1 of them. With
C edges per chunk, three hub sources have 9 C, 9 C + 1 and 17 C + 5 edges: 8 partial rows (exactly one batch), 9 (one row
into a second batch) and 17 (a ragged third batch). Around them: sources with one edge and with none, on both sides of
n_dst. Every target's edge range is shorter than C. Shared by the long-run case of each op's GPU test."""
import numpy as np

N_DST, N_SRC = 300, 420
HUBS = (7, N_DST + 50, 123)          # a target, a source that is no target, a target
SINGLES = (0, 299, N_DST, N_SRC - 1)


def run_lengths(C):
    return (9 * C, 9 * C + 1, 17 * C + 5)


def long_run_block(rng, C):
    """row_ptr [N_DST + 1] int32, col [E] int32: the hubs' edges and the singles, shuffled over the targets"""
    col = np.concatenate([np.full(n, h, np.int32) for h, n in zip(HUBS, run_lengths(C))] + [np.array(SINGLES, np.int32)])
    rng.shuffle(col)
    E = len(col)
    cuts = np.arange(1, N_DST) * E // N_DST + rng.integers(-E // (4 * N_DST), E // (4 * N_DST) + 1, N_DST - 1)
    cuts[1::9] = cuts[0::9][:len(cuts[1::9])]   # every ninth target is empty
    row_ptr = np.concatenate([[0], cuts, [E]]).astype(np.int32)
    assert (np.diff(row_ptr) >= 0).all()
    return row_ptr, col


def assert_long_runs(row_ptr, col, C):
    """the case keeps its point: the three runs have 8, 9 and 17 partial rows, every target's range is below one chunk"""
    counts = np.bincount(col, minlength=N_SRC)
    assert tuple(int(counts[h]) for h in HUBS) == run_lengths(C)
    assert [(int(counts[h]) + C - 1) // C - 1 for h in HUBS] == [8, 9, 17]
    assert all(counts[s] == 1 for s in SINGLES)
    assert (counts[:N_DST] == 0).any() and (counts[N_DST:] == 0).any()
    deg = np.diff(row_ptr)
    assert deg.min() == 0 and 0 < deg.max() < C and len(row_ptr) == N_DST + 1 and row_ptr[-1] == len(col)
