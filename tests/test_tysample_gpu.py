"""Per-relation fan-out sampling on the MI355X (csrc/kernels/tysample.hip through GraphStructure.typed_sample_one_hop) against
the definition restated in numpy (tests/_tysample_ref.py), bit for bit, on the typed ladder: rows of 0, 1, 2, 63, 64, 65, 1024,
1025 and 5000 neighbours, one skewed, one of a single relation, one with types -1 and R, one with exactly f_r edges of a relation."""
import types

import numpy as np
import pytest

import _tysample_ref as ref
from test_tsample_gpu import NP_OF, _destroy, _dev, _structure

pytestmark = pytest.mark.gpu
FLAGS = ((True, True, True), (False, False, False), (True, False, True), (False, True, False))


def _typed_structure(comm, mt="chunked", loc="cuda", col_dtype=np.int64, graph=None):
    row_ptr, col, ty, _ = graph or ref.typed_ladder()
    return _structure(comm, mt, loc, col_dtype, row_ptr, col, ty)      # (the edge attribute is named "t")


def _assert_equal(got, want, flags, what):
    """got: the op's tuple; want: the reference's (offsets, ids, center local ids, edge ids, edge types, ...)"""
    expect = [want[0], want[1]] + [want[2 + k] for k in range(3) if flags[k]]
    assert len(got) == len(expect), what
    for k, (a, b) in enumerate(zip(got, expect)):
        assert a.is_cuda and tuple(a.shape) == b.shape and (k == 1 or a.cpu().numpy().dtype == b.dtype), (k, what)
        assert np.array_equal(a.cpu().numpy().astype(np.int64), b.astype(np.int64)), "output %d differs: %s" % (k, what)


def _sample(g, centres, fanouts, flags=FLAGS[0], seed=ref.LADDER_SEED):
    return g.typed_sample_one_hop("t", centres, fanouts, random_seed=seed, need_center_local_output=flags[0],
                                  need_edge_output=flags[1], need_type_output=flags[2])


@pytest.mark.parametrize("mt,loc", [("continuous", "cuda"), ("chunked", "cuda"), ("continuous", "cpu"), ("chunked", "cpu")])
@pytest.mark.parametrize("center_dtype,col_dtype", [("int64", "int64"), ("int32", "int32"), ("int64", "int32"), ("int32", "int64")])
def test_the_ladder_sample_equals_the_reference(gpu_env, mt, loc, center_dtype, col_dtype):
    print("the typed ladder at %s: %s" % (ref.LADDER_FANOUTS, ref.assert_ladder_measures()))      # (the cases, and 8 of each on the skewed row)
    g, ts = _typed_structure(gpu_env, mt, loc, NP_OF[col_dtype])
    centres = _dev(ref.typed_ladder()[3], NP_OF[center_dtype])
    for flags in FLAGS if (mt, loc) == ("chunked", "cuda") else FLAGS[:1]:
        _assert_equal(_sample(g, centres, ref.LADDER_FANOUTS, flags), ref.ladder_sample(), flags,
                      "%s / %s, centres %s, col %s, outputs %s" % (mt, loc, center_dtype, col_dtype, flags))
    _destroy(ts)


@pytest.mark.parametrize("fanouts", [[64], [1] * 64, [32, 32], [3, 0, 5], [16, 16], [1], [31, 1, 32]], ids=str)
def test_fanout_vectors(gpu_env, fanouts):
    g, ts = _typed_structure(gpu_env)
    _assert_equal(_sample(g, _dev(ref.typed_ladder()[3]), fanouts), ref.ladder_sample(fanouts), FLAGS[0], str(fanouts))
    _destroy(ts)


@pytest.mark.parametrize("m", [1, 32, 33, 64])
def test_one_relation_is_the_temporal_sampler_with_every_edge_eligible(gpu_env, m):
    import torch
    row_ptr, col, _, starts = ref.typed_ladder()
    g, ts = _typed_structure(gpu_env, graph=(row_ptr, col, np.zeros(col.shape[0], np.int32), None))
    h, hs = _structure(gpu_env, "chunked", "cuda", np.int64, row_ptr, col, np.zeros(col.shape[0], np.int64))
    centres = _dev(starts)
    got = _sample(g, centres, [m], (True, True, False))
    want = h.temporal_sample_one_hop("t", centres, torch.zeros_like(centres), m, random_seed=ref.LADDER_SEED,
                                     need_center_local_output=True, need_edge_output=True)
    assert len(got) == len(want) == 4 and all(torch.equal(a, b) for a, b in zip(got, want)) and got[0][-1] > 400
    _destroy(ts + hs)


def test_geometry_damage_and_no_centres(gpu_env):
    """the first 100 centres alone; 70 001, more than the capped grids hold (2048 x 16 and x 8); no nodes; none; damaged rows"""
    import torch
    g, ts = _typed_structure(gpu_env)
    starts, want = ref.typed_ladder()[3], ref.ladder_sample()
    cut = int(want[0][100])
    _assert_equal(_sample(g, _dev(starts[:100]), ref.LADDER_FANOUTS), (want[0][:101],) + tuple(w[:cut] for w in want[1:5]), FLAGS[0], "100")
    centres = np.tile(starts, 137)[:70001]      # (a tiled position has its own streams: the reference is made for all of them)
    tiled = ref.typed_sample(*ref.typed_ladder()[:3], centres, list(ref.LADDER_FANOUTS), ref.LADDER_SEED, draw=ref.fast_draws)
    assert centres.shape[0] == 70001 > 2048 * 16 and tiled[0][-1] > 400000
    _assert_equal(_sample(g, _dev(centres, np.int32), ref.LADDER_FANOUTS), tiled, FLAGS[0], "70 001 centres")
    refused = torch.tensor([-1, 2000, -7, (1 << 31) - 1, 1 << 40], dtype=torch.int64, device="cuda")
    got = _sample(g, refused, [2, 2])
    assert got[0].tolist() == [0] * 6 and all(t.numel() == 0 for t in got[1:])
    got = _sample(g, torch.empty(0, dtype=torch.int32, device="cuda"), [2, 2])
    assert got[0].tolist() == [0] and [(t.numel(), t.dtype) for t in got[1:]] == [
        (0, torch.int64), (0, torch.int32), (0, torch.int64), (0, torch.int32)]
    _destroy(ts)
    row_ptr = np.array([0, 3, 2, 5, 9, 7], dtype=np.int64)      # rows: [0, 3), (3, 2) damaged, [2, 5), (5, 9) and (9, 7) damaged
    col, ty = np.array([1, 2, 0, 4, 3, 0, 2], dtype=np.int64), np.array([0, 1, 0, 0, 1, 0, 0], dtype=np.int32)
    centres = np.array([4, 3, 2, 1, 0, 2], dtype=np.int64)
    want = ref.typed_sample(row_ptr, col, ty, centres, [1, 2], 5)
    assert np.diff(want[0]).tolist() == [0, 0, 2, 0, 2, 2]
    g, ts = _typed_structure(gpu_env, "continuous", graph=(row_ptr, col, ty, None))
    _assert_equal(_sample(g, _dev(centres), [1, 2], seed=5), want, FLAGS[0], "damaged row_ptr")
    _destroy(ts)


def test_two_typed_layers_and_the_rgcn_model(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import graph_ops
    g, ts = _typed_structure(gpu_env, col_dtype=np.int64)
    seeds, fanouts = _dev(np.arange(40)), [[4, 4, 4, 4], [2, 0, 3, 1]]
    gids, edge_indice, row_ptrs, col_inds, attrs = g.multilayer_typed_sample(seeds, fanouts, "t", random_seeds=[11, 12])
    frontier = seeds
    for depth, layer in enumerate((1, 0)):      # by hand: the one-hop op, then append_unique
        off, nbr, lid, ety = _sample(g, frontier, fanouts[depth], (True, False, True), seed=11 + depth)
        widened, pos = graph_ops.append_unique(frontier, nbr, need_neighbor_raw_to_unique=True)
        for a, b in ((gids[layer], widened), (gids[layer + 1], frontier), (row_ptrs[layer], off), (col_inds[layer], pos),
                     (edge_indice[layer], torch.stack([pos, lid])), (attrs[layer]["t"], ety)):
            assert torch.equal(a, b), (depth, a, b)
        frontier = widened
    assert len(gids) == 3 and ety.numel() > 40 and set(ety.tolist()) <= {0, 2, 3}
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [2000, 16])
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(torch.randn(2000, 16, generator=torch.Generator().manual_seed(5)).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    torch.cuda.synchronize()
    wgth.set_framework("cugraph")
    args = types.SimpleNamespace(hiddensize=16, layernum=2, model="rgcn", classnum=5, dropout=0.0, neighbors="5,5", num_relations=4,
                                 edge_type_name="t", relation_fanouts=fanouts)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    model.train()
    out = model(torch.arange(40))
    assert tuple(out.shape) == (40, 5)
    out.square().sum().backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert grads and all(gr is not None and torch.isfinite(gr).all() for gr in grads) and any(gr.abs().sum() > 0 for gr in grads)
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    _destroy(ts)
