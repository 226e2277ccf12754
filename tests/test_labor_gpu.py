"""LABOR layer-neighbour sampling on the MI355X (csrc/kernels/labor.hip through GraphStructure.labor_sample_one_hop) against the
definition restated in numpy (tests/_labor_ref.py), bit for bit, on the LABOR ladder: rows of 0, 1, M - 1, M, M + 1 for every M
used, 129 and 1000 neighbours, a row of multi-edges, a node in every fourth entry, damaged rows, centres that are no node."""
import numpy as np
import pytest

import _labor_ref as ref
from test_tsample_gpu import NP_OF, _destroy, _dev, _structure

pytestmark = pytest.mark.gpu
FLAGS = ((True, True), (False, False), (True, False), (False, True))
CASES = [(m, "fixed") for m in (1, 5, 32, 33, 64, -1)] + [(m, "poisson") for m in (1, 10, 100)]


def _graph(comm, mt="chunked", loc="cuda", col_dtype=np.int64, row_ptr=None, col=None):
    if row_ptr is None:
        row_ptr, col, _ = ref.labor_ladder()
    return _structure(comm, mt, loc, col_dtype, row_ptr, col, np.zeros(len(col), np.int64))      # (the edge attribute is unused)


def _sample(g, centres, m, mode, flags=FLAGS[0], seed=ref.LADDER_SEED):
    return g.labor_sample_one_hop(centres, m, mode=mode, random_seed=seed, need_center_local_output=flags[0], need_edge_output=flags[1])


def _assert_equal(got, want, flags, what):
    expect = [want[0], want[1]] + [want[2 + k] for k in range(2) if flags[k]]
    assert len(got) == len(expect), what
    for k, (a, b) in enumerate(zip(got, expect)):
        assert a.is_cuda and tuple(a.shape) == b.shape and (k == 1 or a.cpu().numpy().dtype == b.dtype), (k, what)
        assert np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)), "output %d differs: %s" % (k, what)


@pytest.mark.parametrize("mt,loc", [("continuous", "cuda"), ("chunked", "cuda"), ("continuous", "cpu"), ("chunked", "cpu")])
@pytest.mark.parametrize("center_dtype,col_dtype", [("int64", "int64"), ("int32", "int32"), ("int64", "int32"), ("int32", "int64")])
def test_the_ladder_sample_equals_the_reference(gpu_env, mt, loc, center_dtype, col_dtype):
    ids = [0, 7, 299, -1, (1 << 31) - 1, -(1 << 31), 1 << 40]
    assert [ref.variate(9, c) for c in ids] == ref.variates(9, ids).tolist()      # the vectorised variate is the scalar one
    g, ts = _graph(gpu_env, mt, loc, NP_OF[col_dtype])
    centres = _dev(ref.labor_ladder()[2], NP_OF[center_dtype])
    for m, mode in CASES:
        for flags in FLAGS if (mt, loc) == ("chunked", "cuda") else FLAGS[:1]:
            _assert_equal(_sample(g, centres, m, mode, flags), ref.ladder_sample(m, mode), flags,
                          "%s / %s, centres %s, col %s, M = %d %s, outputs %s" % (mt, loc, center_dtype, col_dtype, m, mode, flags))
    _destroy(ts)


def test_rows_of_the_same_nodes_overlap(gpu_env):
    """the contract's point, on the op's output alone: rows 0 and 1 hold the same 50 nodes in two orders, row 2 twenty of them"""
    rng = np.random.default_rng(3)
    nodes = rng.choice(10 ** 6, 50, replace=False)
    col = np.concatenate([nodes, rng.permutation(nodes), rng.permutation(nodes)[:20]]).astype(np.int64)
    g, ts = _graph(gpu_env, row_ptr=np.array([0, 50, 100, 120], np.int64), col=col)
    for seed in range(8):
        off, ids = (t.cpu().numpy() for t in _sample(g, _dev([0, 1, 2]), 10, "fixed", FLAGS[1], seed))
        assert off.tolist() == [0, 10, 20, 30] and set(ids[:10]) == set(ids[10:20])
        off, ids = (t.cpu().numpy() for t in _sample(g, _dev([0, 1, 2]), 10, "poisson", FLAGS[1], seed))
        long_row, short_row = set(ids[:off[1]]), set(ids[off[2]:])
        assert long_row == set(ids[off[1]:off[2]]) and long_row & set(col[100:]) <= short_row      # (10 / 50 < 10 / 20)
    _destroy(ts)


@pytest.mark.parametrize("m,mode", [(5, "fixed"), (3, "poisson")])
def test_geometry_and_no_centres(gpu_env, m, mode):
    """the first 100 centres alone; 525 001 centres of at most 8 neighbours, more than any capped grid holds (2048 x 256); none"""
    import torch
    g, ts = _graph(gpu_env)
    row_ptr, col, centres = ref.labor_ladder()
    want = ref.ladder_sample(m, mode)
    cut = int(want[0][100])
    _assert_equal(_sample(g, _dev(centres[:100]), m, mode), (want[0][:101],) + tuple(w[:cut] for w in want[1:]), FLAGS[0], "100")
    small = np.concatenate([np.arange(23, 302), [-1, 5]]).astype(np.int64)      # (5: M + 1 entries in fixed mode)
    reps = 525001 // small.shape[0] + 1
    many = ref.tiled(ref.labor_sample(row_ptr, col, small, m, mode, ref.LADDER_SEED), small.shape[0], reps)
    end = int(many[0][525001])
    assert np.diff(row_ptr)[23:300].max() <= 8 and 525001 > 2048 * 256 and end > 10 ** 6
    _assert_equal(_sample(g, _dev(np.tile(small, reps)[:525001], np.int32), m, mode), (many[0][:525002],) + tuple(w[:end] for w in many[1:]),
                  FLAGS[0], "525 001 centres")
    got = _sample(g, torch.empty(0, dtype=torch.int32, device="cuda"), m, mode)
    assert got[0].tolist() == [0] and [(t.numel(), t.dtype) for t in got[1:]] == [(0, torch.int64), (0, torch.int32), (0, torch.int64)]
    _destroy(ts)


@pytest.mark.parametrize("mode", ["fixed", "poisson"])
@pytest.mark.parametrize("layer_dependency", [False, True])
def test_two_layers_equal_the_reference_hop_by_hop(gpu_env, mode, layer_dependency):
    import torch
    from wholegraph_amd.torch import graph_ops
    g, ts = _graph(gpu_env)
    row_ptr, col, _ = ref.labor_ladder()
    seeds, fanouts, rs = _dev(np.arange(40)), [3, 2], [11] if layer_dependency else [11, 12]
    gids, edge_indice, row_ptrs, col_inds = g.multilayer_labor_sample(seeds, fanouts, mode=mode, layer_dependency=layer_dependency,
                                                                      random_seeds=rs)
    frontier = seeds
    for depth, layer in enumerate((1, 0)):      # the reference's hop, then append_unique
        off, nbr, lid, _ = ref.labor_sample(row_ptr, col, frontier.cpu().numpy(), fanouts[depth], mode, rs[0 if layer_dependency else depth])
        widened, pos = graph_ops.append_unique(frontier, _dev(nbr), need_neighbor_raw_to_unique=True)
        for a, b in ((gids[layer], widened), (gids[layer + 1], frontier), (row_ptrs[layer], _dev(off, np.int32)), (col_inds[layer], pos),
                     (edge_indice[layer], torch.stack([pos, _dev(lid, np.int32)]))):
            assert torch.equal(a, b), (depth, a, b)
        frontier = widened
    assert len(gids) == 3 and gids[0].numel() > gids[1].numel() > 40
    _destroy(ts)
