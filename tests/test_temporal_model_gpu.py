"""Temporal sampling end to end on the MI355X: GraphStructure.multilayer_temporal_sample on the temporal ladder
(tests/_tsample_ref.py) with fan-outs [5, 5] under both propagate modes — no edge of any hop lies in the future of its tree's
time, checked on the host from the edge ids; the shapes are those of the tree definition; hop 0 equals the one-hop reference —
and TemporalGNNModel (wholegraph_amd/torch/temporal.py): forward and backward with finite gradients in every parameter, the same
seeds giving the same logits twice."""
import types

import numpy as np
import pytest

import _tsample_ref as ref

pytestmark = pytest.mark.gpu

FANOUTS, SEEDS = [5, 5], [101, 202]
N, DIM, CLASSES = 2000, 32, 5


def _wm_array(comm, mt, arr):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr))


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm):
    import wholegraph_amd.torch as wgth
    row_ptr, col, etime, _, _ = ref.temporal_ladder()
    ts = [_wm_array(comm, "chunked", row_ptr), _wm_array(comm, "chunked", col), _wm_array(comm, "chunked", etime)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("t", ts[2])
    return g, ts


def _batch():
    """the ladder's batch without its three ids that are no nodes, and without the INT64_MIN / INT64_MAX centre times (the
    model subtracts times)"""
    import torch
    _, _, _, starts, ctimes = ref.temporal_ladder()
    keep = (starts >= 0) & (starts < N) & (np.abs(ctimes) < (1 << 40))
    return torch.from_numpy(starts[keep]).cuda(), torch.from_numpy(ctimes[keep]).cuda()


@pytest.mark.parametrize("inclusive,window", [(True, None), (False, 50)])
@pytest.mark.parametrize("propagate", ["seed", "edge"])
def test_no_edge_of_any_hop_lies_in_its_trees_future(gpu_env, propagate, inclusive, window):
    import torch
    row_ptr, col, etime, starts, ctimes = ref.temporal_ladder()
    g, ts = _structure(gpu_env)
    seeds, seed_times = torch.from_numpy(np.array(starts)).cuda(), torch.from_numpy(np.array(ctimes)).cuda()
    out = g.multilayer_temporal_sample(seeds, seed_times, FANOUTS, "t", inclusive=inclusive, time_window=window, propagate=propagate,
                                       random_seeds=SEEDS, edge_attr_names=["t", "__edge_id__"])
    assert len(out) == 7
    gids, gtimes, edge_indice, row_ptrs, col_inds, edge_ids, attrs = [[t.cpu().numpy() if torch.is_tensor(t) else t for t in part]
                                                                     for part in out]
    hops = len(FANOUTS)
    assert [len(part) for part in out] == [hops + 1, hops + 1, hops, hops, hops, hops, hops]
    assert np.array_equal(gids[-1], starts) and np.array_equal(gtimes[-1], ctimes)
    total = 0
    for layer in range(hops - 1, -1, -1):      # from the seeds outwards
        centres, times = gids[layer + 1], gtimes[layer + 1]
        n_c, n_e = centres.shape[0], edge_ids[layer].shape[0]
        offsets, lid = row_ptrs[layer].astype(np.int64), edge_indice[layer][1].astype(np.int64)
        # the shapes of the tree definition
        assert offsets.shape == (n_c + 1,) and offsets[0] == 0 and offsets[-1] == n_e and (np.diff(offsets) <= FANOUTS[hops - 1 - layer]).all()
        assert col_inds[layer].dtype == np.int32 and np.array_equal(col_inds[layer], n_c + np.arange(n_e))
        assert edge_indice[layer].shape == (2, n_e) and np.array_equal(edge_indice[layer][0], col_inds[layer])
        assert np.array_equal(lid, np.repeat(np.arange(n_c), np.diff(offsets)))
        assert gids[layer].shape == (n_c + n_e,) and np.array_equal(gids[layer][:n_c], centres) and np.array_equal(gtimes[layer][:n_c], times)
        # every edge is an edge of its centre, and passes the rule against its tree's time
        eid = edge_ids[layer]
        u = centres[lid]
        assert ((eid >= row_ptr[u]) & (eid < row_ptr[u + 1])).all() and np.array_equal(gids[layer][n_c:], col[eid])
        assert all(ref.eligible(int(ts_), int(t), inclusive, window) for ts_, t in zip(etime[eid], times[lid])), "an edge from the future"
        inherited = times[lid] if propagate == "seed" else etime[eid]
        assert np.array_equal(gtimes[layer][n_c:], inherited)
        assert np.array_equal(attrs[layer]["t"].cpu().numpy(), etime[eid]) and np.array_equal(attrs[layer]["__edge_id__"].cpu().numpy(), eid)
        total += n_e
    # hop 0 is the one-hop sampler's answer
    want = ref.temporal_sample(row_ptr, col, etime, starts, ctimes, FANOUTS[0], "uniform", inclusive, window, SEEDS[0], draw=ref.cached_draws)
    assert np.array_equal(row_ptrs[-1], want[0]) and np.array_equal(edge_ids[-1], want[3])
    assert want[0][-1] >= 150 and total >= want[0][-1] + 50, "the trees are too small to show anything"
    six = g.multilayer_temporal_sample(seeds, seed_times, FANOUTS, "t", inclusive=inclusive, time_window=window, propagate=propagate,
                                       random_seeds=SEEDS)
    assert len(six) == 6 and all(torch.equal(a, b) for part, other in zip(six, out) for a, b in zip(part, other))
    _destroy(ts)


def _model(comm, propagate):
    import torch
    import wholegraph_amd.torch as wgth
    g, ts = _structure(comm)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [N, DIM])
    table = torch.randn(N, DIM, generator=torch.Generator().manual_seed(3))
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(table.cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    torch.cuda.synchronize()
    wgth.set_framework("cugraph")
    torch.manual_seed(5)
    args = types.SimpleNamespace(hiddensize=64, layernum=2, classnum=CLASSES, dropout=0.0, heads=2, neighbors="5,5", time_dim=16,
                                 temporal_propagate=propagate)
    model = wgth.TemporalGNNModel(g, emb, args, "t").cuda()

    def done():
        wgth.destroy_wholememory_optimizer(wm_opt)
        wgth.destroy_embedding(emb)
        _destroy(ts)
    return model, emb, done


@pytest.mark.parametrize("propagate", ["seed", "edge"])
def test_model_forward_backward_and_the_same_logits_twice(gpu_env, propagate):
    import torch
    import torch.nn.functional as F
    model, emb, done = _model(gpu_env, propagate)
    assert [type(l).__name__ for l in model.gnn_layers] == ["EdgeGATConv"] * 2
    assert [(l.heads, l.concat, l.out_channels, l.edge_dim) for l in model.gnn_layers] == [(2, True, 32, 16), (2, False, CLASSES, 16)]
    seeds, seed_times = _batch()
    assert seeds.shape[0] >= 500
    model.train()
    logits = model(seeds, seed_times, random_seeds=SEEDS)
    assert tuple(logits.shape) == (seeds.shape[0], CLASSES) and torch.isfinite(logits).all()
    loss = F.cross_entropy(logits, (seeds % CLASSES).long())
    loss.backward()
    assert torch.isfinite(loss)
    assert len(emb.sparse_grads) == 1 and torch.isfinite(emb.sparse_grads[0]).all() and (emb.sparse_grads[0] != 0).any()
    params = dict(model.named_parameters())
    assert {"time_encoder.lin.weight", "time_encoder.lin.bias", "gnn_layers.0.lin_edge.weight", "self_layers.1.weight"} <= set(params)
    for pname, p in params.items():
        if not p.requires_grad:      # (the embedding's autograd anchor)
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any(), pname
    with torch.no_grad():
        again = model(seeds, seed_times, random_seeds=SEEDS)
        other = model(seeds, seed_times, random_seeds=[7, 8])
    assert torch.equal(again, logits.detach()), "the same seeds, other logits"
    assert not torch.equal(other, again), "other seeds, the same logits"
    done()
