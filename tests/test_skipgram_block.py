"""skipgram_block and centers_of (wholegraph_amd/torch/skipgram.py) on CPU tensors against the plain-loop restatement of
tests/_skipgram_ref.py: all four outputs equal exactly, on walks that end early, hold no node, or have a hole in the middle;
the number of edges is the one the definition gives; a block of 2^31 edges or more is refused before it is built."""
import numpy as np
import pytest

import _skipgram_ref as ref

L = 6


def hand_walks(dtype):
    """a full walk; walks cut after 1, 2 and L nodes; an all -1 row; a -1 in the middle of a row; a repeated node"""
    rows = [[10, 11, 12, 13, 14, 15, 16],
            [20, -1, -1, -1, -1, -1, -1],
            [30, 31, -1, -1, -1, -1, -1],
            [40, 41, 42, 43, 44, 45, -1],
            [-1, -1, -1, -1, -1, -1, -1],
            [50, 51, -1, 53, 54, -1, 56],
            [7, 8, 7, 7, 9, 8, 7]]
    return np.array(rows, dtype)


def hand_negatives(n_centers, K, dtype):
    rng = np.random.default_rng(5)
    neg = rng.integers(0, 100, (n_centers, K)).astype(dtype)
    neg[rng.random((n_centers, K)) < 0.3] = -1
    neg[0, :] = -1
    return neg


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("W", [1, 3, L + 2])
@pytest.mark.parametrize("K", [None, 1, 4])
def test_block_equals_the_loop_restatement(wm_lib, dtype, W, K):
    import torch
    from wholegraph_amd.torch.skipgram import centers_of, skipgram_block
    walks = hand_walks(dtype)
    centers = centers_of(torch.from_numpy(walks))
    want_centers = walks[walks >= 0]
    assert centers.dtype == torch.from_numpy(walks).dtype and np.array_equal(centers.numpy(), want_centers)
    neg = None if K is None else hand_negatives(len(want_centers), K, dtype)
    got = skipgram_block(torch.from_numpy(walks), W, None if neg is None else torch.from_numpy(neg))
    want = ref.skipgram_block_ref(walks, W, neg)
    for g, w, name in zip(got, want, ("center_ids", "row_ptr", "ctx_ids", "labels")):
        assert g.numpy().dtype == w.dtype and np.array_equal(g.numpy(), w), name
    assert got[1].dtype == torch.int32 and got[3].dtype == torch.float32
    assert len(got[2]) == int(got[1][-1]) == ref.edge_count(walks, W, neg)
    assert (got[2] >= 0).all()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_no_walk_and_a_walk_of_no_step(wm_lib, dtype):
    import torch
    from wholegraph_amd.torch.skipgram import centers_of, skipgram_block
    empty = torch.from_numpy(np.zeros((0, L + 1), dtype))
    assert centers_of(empty).shape == (0,)
    for neg in (None, torch.from_numpy(np.zeros((0, 3), dtype))):
        c, rp, ctx, lab = skipgram_block(empty, 2, neg)
        assert c.shape == (0,) and rp.tolist() == [0] and ctx.shape == (0,) and lab.shape == (0,)
        assert c.dtype == empty.dtype and ctx.dtype == empty.dtype
    starts = np.array([[4], [-1], [6]], dtype)   # L = 0: no positive anywhere
    neg = np.array([[1, -1], [2, 3]], dtype)
    got = skipgram_block(torch.from_numpy(starts), 3, torch.from_numpy(neg))
    want = ref.skipgram_block_ref(starts, 3, neg)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    assert got[1].tolist() == [0, 1, 3] and got[3].tolist() == [0.0, 0.0, 0.0]


def test_random_walks_against_the_restatement(wm_lib):
    import torch
    from wholegraph_amd.torch.skipgram import skipgram_block
    rng = np.random.default_rng(11)
    walks = rng.integers(0, 50, (40, 9)).astype(np.int64)
    ends = rng.integers(0, 10, 40)
    walks[np.arange(9)[None, :] >= ends[:, None]] = -1
    neg = rng.integers(-1, 50, (int((walks >= 0).sum()), 5)).astype(np.int64)
    got = skipgram_block(torch.from_numpy(walks), 2, torch.from_numpy(neg))
    want = ref.skipgram_block_ref(walks, 2, neg)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))


def test_arguments(wm_lib):
    import torch
    from wholegraph_amd.torch.skipgram import centers_of, skipgram_block
    walks = torch.from_numpy(hand_walks(np.int64))
    with pytest.raises(ValueError, match="window"):
        skipgram_block(walks, 0)
    with pytest.raises(ValueError, match="L \\+ 1"):
        skipgram_block(walks.reshape(-1), 1)
    with pytest.raises(TypeError, match="int32 or int64"):
        centers_of(walks.float())
    with pytest.raises(ValueError, match="row per centre"):
        skipgram_block(walks, 1, torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(TypeError, match="int32 or int64"):
        skipgram_block(walks, 1, torch.zeros((int((walks >= 0).sum()), 2)))


def test_2_to_the_31_edges_are_refused_before_the_block_is_built(wm_lib, monkeypatch):
    """by arithmetic on the shapes: the bound of a batch that cannot reach 2^31 edges lets it through uncounted; one that
    could is counted first (the count mocked here: no such batch is allocated) and refused without building anything"""
    import torch
    from wholegraph_amd.torch import skipgram as sg
    assert sg._edge_count_bound(1000 * 81, 5, 5) == 81000 * 15 < 2 ** 31
    assert sg._edge_count_bound(2 ** 20 * 129, 10, 5) >= 2 ** 31        # 2^20 walks of 128 steps, W = 10, K = 5
    walks = torch.from_numpy(hand_walks(np.int64))
    neg = torch.from_numpy(hand_negatives(int((walks >= 0).sum()), 2, np.int64))
    exact = sg._exact_edge_count(walks, min(3, L), neg)
    assert exact == ref.edge_count(walks.numpy(), 3, neg.numpy()) == len(sg.skipgram_block(walks, 3, neg)[2])
    counted = []
    monkeypatch.setattr(sg, "_edge_count_bound", lambda *a: 2 ** 31)
    monkeypatch.setattr(sg, "_exact_edge_count", lambda *a: counted.append(a) or exact)
    assert len(sg.skipgram_block(walks, 3, neg)[2]) == exact and len(counted) == 1   # counted, below the limit: built
    monkeypatch.setattr(sg, "_exact_edge_count", lambda *a: 2 ** 31)
    monkeypatch.setattr(torch, "cat", lambda *a, **k: pytest.fail("the block was being built"))
    with pytest.raises(ValueError, match="2\\^31"):
        sg.skipgram_block(walks, 3, neg)
    monkeypatch.setattr(sg, "_exact_edge_count", lambda *a: 2 ** 31 - 1)
    with pytest.raises(pytest.fail.Exception):
        sg.skipgram_block(walks, 3, neg)     # one below the limit goes on to build
