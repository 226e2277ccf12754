"""The block of tests/_capped_block.py keeps its point (no GPU needed): from numpy alone, every property that makes a launch
under WM_AGG_MAX_BLOCKS = 1 or 3 take a second, a late and a ragged trip of its grid-stride loop at every lane width."""
import numpy as np

import _capped_block as CB

GROUPS_PER_BLOCK = (16, 8, 4)   # 256 lanes in groups of 16, 32 and 64
CAPS = (1, 3)


def _block(wm_lib):
    from wholegraph_amd.torch.aggregation import chunk_edges
    C = chunk_edges()
    assert C >= 1
    return (C,) + CB.capped_block(C)


def test_sizes_make_every_last_trip_ragged(wm_lib):
    C, row_ptr, col = _block(wm_lib)
    assert len(row_ptr) == CB.N_DST + 1 == 302 and CB.N_SRC == 1103
    assert row_ptr[0] == 0 and row_ptr[-1] == len(col) and (np.diff(row_ptr) >= 0).all()
    assert col.min() >= 0 and col.max() < CB.N_SRC
    for n in (CB.N_DST, CB.N_SRC):
        for g in GROUPS_PER_BLOCK:
            for cap in CAPS:
                assert n % (g * cap) != 0, (n, g, cap)      # the last trip is ragged ...
                assert n > 2 * g * cap, (n, g, cap)         # ... and it is at least the third
    E = len(col)
    assert E >= CB.min_edges(C) == 20 * C + 3
    assert 30 <= E / CB.N_DST <= 40
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    assert (CB.N_SRC + node_chunk() - 1) // node_chunk() == 2   # two node chunks of the attention ops' grad_att
    n_tiles = (E + C - 1) // C
    assert n_tiles > CB.MIN_TILES == max(GROUPS_PER_BLOCK)
    assert row_ptr.flags.writeable is False and col.flags.writeable is False
    assert CB.capped_block(C)[0] is row_ptr                 # built once


def test_boundary_degrees_on_the_first_and_on_a_late_ragged_trip(wm_lib):
    C, row_ptr, col = _block(wm_lib)
    deg = np.diff(row_ptr)
    nb = len(CB.BOUNDARY_DEGREES)
    assert CB.BOUNDARY_DEGREES == (0, 1, 8, 9, 17, 65)
    assert tuple(deg[:nb]) == CB.BOUNDARY_DEGREES
    assert tuple(deg[-nb:]) == CB.BOUNDARY_DEGREES
    # (targets 0 .. 3 are the first trip of a 64-lane kernel under cap 1, 0 .. 7 that of the 16- and 32-lane kernels; the
    # last six are a third or later trip, the last of them ragged, at every lane width: test_sizes_... checks the sizes)
    assert (deg[nb:-nb] >= 25).all() and deg.max() == 65


def test_hubs_and_their_chunk_tiles(wm_lib):
    C, row_ptr, col = _block(wm_lib)
    counts = np.bincount(col, minlength=CB.N_SRC)
    assert CB.EARLY_HUB == 0 and counts[CB.EARLY_HUB] == C + 1
    assert CB.LATE_HUB == CB.N_SRC - 1 and counts[CB.LATE_HUB] == 2 * C + 3
    assert (np.delete(counts, [CB.EARLY_HUB, CB.LATE_HUB]) <= C).all()   # no other run is chunked
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(CB.N_SRC + 1))
    assert starts[CB.EARLY_HUB] == 0                                    # the early hub's run opens the sorted positions:
    assert (starts[CB.EARLY_HUB] + C) // C == 1                         # its chunk 1 starts in tile 1, on the first trip
    s0, s1 = starts[CB.LATE_HUB], starts[CB.LATE_HUB + 1]
    assert s1 == len(col) and s1 - s0 == 2 * C + 3                      # the late hub's run closes them
    chunk_starts = [s0 + k * C for k in (1, 2)]
    assert all(cs < s1 for cs in chunk_starts)
    assert all(cs // C >= CB.MIN_TILES for cs in chunk_starts), [cs // C for cs in chunk_starts]
    assert len({cs // C for cs in chunk_starts}) == 2


def test_duplicate_edges_and_sources_without_edges(wm_lib):
    C, row_ptr, col = _block(wm_lib)
    counts = np.bincount(col, minlength=CB.N_SRC)
    assert all(counts[s] == 0 for s in CB.NO_EDGES)
    assert any(s < CB.N_DST for s in CB.NO_EDGES) and any(s >= CB.N_DST for s in CB.NO_EDGES)
    for d in CB.DUPLICATE_IN:
        assert row_ptr[d + 1] - row_ptr[d] >= 2 and col[row_ptr[d]] == col[row_ptr[d] + 1], d
    assert min(CB.DUPLICATE_IN) < 8 and max(CB.DUPLICATE_IN) >= CB.N_DST - 8
    assert (counts[:CB.N_DST] > 0).any() and (counts[CB.N_DST:] > 0).any()
