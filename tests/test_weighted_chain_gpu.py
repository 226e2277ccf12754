"""Weighted neighbour sampling on the small-fan-out kernel, the fused hop and the one-call chain (MI355X). Every comparison is
exact: the one-hop op against the CPU oracle position for position (oracle.sample_weighted restates the contract above
sample_weighted_kernel in csrc/kernels/graph.hip), the fused hop against sampler + append_unique, the chain against the
hop-by-hop route and against a hand-rolled loop over the two ops, the deferred handle against the chain."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 10, 30, 32, 33, 64)      # sample_weighted_small_kernel
LARGE = (65, 300)                       # sample_weighted_kernel, as before
HUB = 3100


def _wm_array(comm, mt, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, mt, "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


def _degree_classes(m):
    return sorted({0, 1, max(m - 1, 0), m, m + 1, 127, 128, 129, HUB})


def _graph(col_dtype, wdtype, n_nodes=3001, seed=5):
    """degrees uniform in [0, 90] plus, at fixed nodes, every class the parity test wants for every fan-out it runs; weights
    10^U(-6, 6) with runs of equal weights (whole rows, half the hub, and every 7th edge)"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 91, n_nodes)
    special = sorted({d for m in SMALL + LARGE for d in _degree_classes(m)})
    nodes = {d: 10 + 3 * k for k, d in enumerate(special)}
    for d, node in nodes.items():
        deg[node] = d
    row_ptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    n_edges = int(row_ptr[-1])
    col = rng.integers(0, n_nodes, n_edges).astype(col_dtype)
    w = np.power(10.0, rng.uniform(-6.0, 6.0, n_edges))
    w[::7] = 1.0
    for node in (nodes[128], nodes[129], nodes[33], 500, 501, 502):
        w[row_ptr[node]:row_ptr[node + 1]] = 0.25
    hub = nodes[HUB]
    w[row_ptr[hub]:row_ptr[hub] + HUB // 2] = 3.0
    return row_ptr, col, w.astype(wdtype), nodes


def _graph_structure(comm, mt, row_ptr, col, weights):
    import wholegraph_amd.torch as wgth
    ts = [_wm_array(comm, mt, a) for a in (row_ptr, col, weights)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("w", ts[2])
    return g, ts


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


@pytest.mark.parametrize("mt", ["continuous", "chunked"])
@pytest.mark.parametrize("wdtype", [np.float32, np.float64])
@pytest.mark.parametrize("center_dtype,col_dtype", [(np.int32, np.int32), (np.int64, np.int64), (np.int64, np.int32),
                                                    (np.int32, np.int64)])
def test_one_hop_equals_the_oracle(gpu_env, mt, wdtype, center_dtype, col_dtype):
    import torch
    row_ptr, col, weights, nodes = _graph(col_dtype, wdtype)
    assert weights.min() < 2e-6 and weights.max() > 5e5
    g, ts = _graph_structure(gpu_env, mt, row_ptr, col, weights)
    rng = np.random.default_rng(17)
    centers = np.concatenate([sorted(nodes.values()), rng.integers(0, row_ptr.shape[0] - 1, 900), [nodes[HUB], nodes[0]]])
    centers = centers.astype(center_dtype)
    deg = row_ptr[centers.astype(np.int64) + 1] - row_ptr[centers.astype(np.int64)]
    for m in SMALL + LARGE:
        for d in _degree_classes(m):       # a generator change cannot silently drop a class
            assert (deg == d).any(), "no centre of degree %d for max_sample_count %d" % (d, m)
        seed = 1234567 * m + 987654321987
        off, ids, lid, egid = g.weighted_sample_without_replacement_one_hop(
            "w", torch.from_numpy(centers).cuda(), m, random_seed=seed, need_center_local_output=True, need_edge_output=True)
        o_off, o_ids, o_lid, o_egid = oracle.sample_weighted(row_ptr, col, weights, centers, m, seed)
        assert np.array_equal(off.cpu().numpy(), o_off), "offsets differ at max_sample_count=%d" % m
        assert np.array_equal(egid.cpu().numpy(), o_egid), "edge ids differ at max_sample_count=%d" % m
        assert np.array_equal(ids.cpu().numpy(), o_ids), "ids differ at max_sample_count=%d" % m
        assert np.array_equal(lid.cpu().numpy(), o_lid), "centre local ids differ at max_sample_count=%d" % m
        # the outputs are optional one by one
        off2, ids2 = g.weighted_sample_without_replacement_one_hop("w", torch.from_numpy(centers).cuda(), m, random_seed=seed)
        assert torch.equal(off2, off) and torch.equal(ids2, ids)
    _destroy(ts)


@pytest.mark.parametrize("mt", ["continuous", "chunked"])
@pytest.mark.parametrize("id_dtype,wdtype", [(np.int32, np.float32), (np.int64, np.float64)])
def test_fused_hop_equals_sampler_plus_append_unique(gpu_env, mt, id_dtype, wdtype):
    import torch
    import wholegraph_amd.torch.graph_ops as gops
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, weights, nodes = _graph(id_dtype, wdtype)
    g, ts = _graph_structure(gpu_env, mt, row_ptr, col, weights)
    csr = (ts[0].wmb_tensor, ts[1].wmb_tensor)
    rng = np.random.default_rng(3)
    frontier = torch.from_numpy(np.concatenate([sorted(nodes.values()), rng.permutation(3001)[:600],
                                                [nodes[HUB]]]).astype(id_dtype)).cuda()
    for m in (1, 10, 30, 33, 64, 65, 300):
        seed = 99 + m
        fused = wops.sample_append_unique(*csr, frontier, m, seed, wm_csr_weight_ptr_tensor=ts[2].wmb_tensor)
        assert fused is not None, "the weighted fused hop was declined at max_sample_count=%d" % m
        off, ids, lid = g.weighted_sample_without_replacement_one_hop("w", frontier, m, random_seed=seed,
                                                                       need_center_local_output=True)
        uniq, pos = gops.append_unique(frontier, ids, need_neighbor_raw_to_unique=True)
        for name, a, b in zip(("offsets", "unique", "neighbor_pos", "center_lid"), fused, (off, uniq, pos, lid)):
            assert a.dtype == b.dtype and torch.equal(a, b), "%s differs at max_sample_count=%d" % (name, m)
    # a frontier of isolated nodes: nothing sampled, the frontier comes back
    lonely = torch.from_numpy(np.array([nodes[0]] * 3, dtype=id_dtype)).cuda()
    off, uniq, pos, lid = wops.sample_append_unique(*csr, lonely, 30, 5, wm_csr_weight_ptr_tensor=ts[2].wmb_tensor)
    assert off.tolist() == [0, 0, 0, 0] and torch.equal(uniq, lonely) and pos.numel() == 0 and lid.numel() == 0
    _destroy(ts)


def _chain_graph(id_dtype, n_nodes=30011):
    from test_graph_oracle import make_csr
    row_ptr, col = make_csr(n_nodes, 60, 7, id_dtype, heavy=[(3, 5000), (4, 0), (5, 1500), (6, 31), (7, 201), (8, 129)])
    rng = np.random.default_rng(23)
    w = np.power(10.0, rng.uniform(-6.0, 6.0, col.shape[0]))
    w[::5] = 2.0
    return row_ptr, col, w.astype(np.float32)


def _assert_same(got, ref):
    import torch
    for name, a_list, b_list in zip(("target_gids", "edge_indice", "csr_row_ptr", "csr_col_ind"), got, ref):
        assert len(a_list) == len(b_list)
        for layer, (a, b) in enumerate(zip(a_list, b_list)):
            assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), "%s[%d]: %s vs %s" % (name, layer, a.shape, b.shape)
            assert torch.equal(a, b), "%s[%d] differs" % (name, layer)


def _hand_rolled(g, seeds, fanouts, hop_seeds):
    """the reference's loop: one-hop weighted sampler + append_unique per hop"""
    import torch
    import wholegraph_amd.torch.graph_ops as gops
    hops = len(fanouts)
    targets, edges, rows, cols = [None] * (hops + 1), [None] * hops, [None] * hops, [None] * hops
    targets[hops] = seeds
    frontier = seeds
    for depth, fanout in enumerate(fanouts):
        layer = hops - 1 - depth
        off, ids, lid = g.weighted_sample_without_replacement_one_hop("w", frontier, fanout, random_seed=hop_seeds[depth],
                                                                       need_center_local_output=True)
        frontier, pos = gops.append_unique(frontier, ids, need_neighbor_raw_to_unique=True)
        targets[layer], edges[layer], rows[layer], cols[layer] = frontier, torch.stack([pos, lid]), off, pos
    return targets, edges, rows, cols


@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("fanouts", [[30], [30, 30], [30, 20, 10]])
def test_chain_equals_hop_by_hop_and_the_two_ops(gpu_env, knobs, monkeypatch, id_dtype, fanouts):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    row_ptr, col, weights = _chain_graph(id_dtype)
    g, ts = _graph_structure(gpu_env, "chunked", row_ptr, col, weights)
    seeds = torch.from_numpy(np.concatenate([[3, 4, 5, 6, 7, 8, 7], np.random.default_rng(9).permutation(30011)[:300]])
                             .astype(id_dtype)).cuda()
    hop_seeds = [77 + 5 * i for i in range(len(fanouts))]
    knobs.set("WM_MULTILAYER_CHAIN", "0")
    ref = g.multilayer_sample_without_replacement(seeds, fanouts, weight_name="w", random_seeds=hop_seeds)
    knobs.set("WM_MULTILAYER_CHAIN", "1")
    # the route: with the chain on, neither the fused hop nor the plain sampler may be called — the whole sample is ONE
    # library call, and the one host synchronise is PendingMultilayerSample.finish's
    calls = {"finish": 0}
    finish = wops.PendingMultilayerSample.finish

    def counted_finish(self):
        calls["finish"] += 1
        return finish(self)

    def forbidden(*a, **k):
        raise AssertionError("the weighted sample left the one-call chain")

    with monkeypatch.context() as mp:
        mp.setattr(wops.PendingMultilayerSample, "finish", counted_finish)
        mp.setattr(wops, "sample_append_unique", forbidden)
        mp.setattr(wops, "weighted_sample_without_replacement", forbidden)
        got = g.multilayer_sample_without_replacement(seeds, fanouts, weight_name="w", random_seeds=hop_seeds)
    assert calls["finish"] == 1
    torch.cuda.synchronize()
    _assert_same(got, ref)
    _assert_same(got, _hand_rolled(g, seeds, fanouts, hop_seeds))
    # its outputs are views of upper-bound buffers
    assert got[0][0].untyped_storage().nbytes() >= ref[0][0].untyped_storage().nbytes()
    # weighted and unweighted samples of the same seeds differ (the weight tensor is really used)
    plain = g.multilayer_sample_without_replacement(seeds, fanouts, random_seeds=hop_seeds)
    assert not all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(plain[0], got[0]))
    _destroy(ts)


@pytest.mark.parametrize("id_dtype,fanouts", [(np.int32, [30, 30]), (np.int64, [7, 5, 3])])
def test_deferred_weighted_chain_feeds_the_gather(gpu_env, id_dtype, fanouts):
    import torch
    import wholegraph_amd.torch as wgth
    n_nodes, dim = 30011, 32
    row_ptr, col, weights = _chain_graph(id_dtype)
    g, ts = _graph_structure(gpu_env, "chunked", row_ptr, col, weights)
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [n_nodes, dim])
    local, _ = emb.get_embedding_tensor().get_local_tensor()
    local.copy_(torch.arange(n_nodes, device="cuda", dtype=torch.float32).unsqueeze(1) + torch.arange(dim, device="cuda") / 64.0)
    seeds = torch.from_numpy(np.concatenate([[3, 4, 5], np.random.default_rng(5).permutation(n_nodes)[:300]]).astype(id_dtype)).cuda()
    hop_seeds = [11 + 3 * i for i in range(len(fanouts))]
    ref = g.multilayer_sample_without_replacement(seeds, fanouts, weight_name="w", random_seeds=hop_seeds)
    h = g.multilayer_sample_begin(seeds, fanouts, random_seeds=hop_seeds, weight_name="w")
    padded = h.padded_frontier
    out = torch.full((padded.shape[0], dim), -7.0, device="cuda")
    emb.gather(padded, out=out)                      # queued behind the sampling kernels, before result()
    got = h.result()
    torch.cuda.synchronize()
    _assert_same(got, ref)
    n = got[0][0].shape[0]
    assert padded.shape[0] > n                       # the chain handed out its upper-bound array
    assert torch.equal(padded[:n], got[0][0]) and bool((padded[n:] == -1).all())
    assert torch.equal(out[:n], emb.gather(got[0][0])) and bool((out[n:] == -7.0).all())
    wgth.destroy_embedding(emb)
    _destroy(ts)


def test_route_taken(gpu_env):
    """what the chain's query mode answers, and what a declined sample falls back to"""
    import torch
    from wholegraph_amd import binding as wmb
    row_ptr, col, weights = _chain_graph(np.int64)
    g, ts = _graph_structure(gpu_env, "chunked", row_ptr, col, weights)
    wint = _wm_array(gpu_env, "chunked", np.ones(col.shape[0], dtype=np.int32))
    wshort = _wm_array(gpu_env, "chunked", np.ones(col.shape[0] - 1, dtype=np.float32))
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    seeds = torch.arange(3, 300, dtype=torch.int64, device="cuda")
    ws = wrap_torch_tensor(seeds)

    def query(weight, fanouts):
        fan = (C.c_int * len(fanouts))(*fanouts)
        return wmb.lib().wholememory_ext_multilayer_sample_weighted(ts[0].wmb_tensor, ts[1].wmb_tensor, weight.wmb_tensor,
                                                                    ws.handle, len(fanouts), fan, None, None, None, None, None,
                                                                    None, None, None)

    assert query(ts[2], [30, 30]) == wmb.WHOLEMEMORY_SUCCESS
    assert query(ts[2], [30, 8193]) == wmb.NOT_SUPPORTED
    assert query(wint, [30, 30]) == wmb.NOT_SUPPORTED
    assert query(wshort, [30, 30]) == wmb.NOT_SUPPORTED
    # the fallback still raises what the plain sampler raises
    with pytest.raises(wmb.WholeMemoryError) as e:
        g.multilayer_sample_without_replacement(seeds, [8193], weight_name="w", random_seeds=[1])
    assert "NOT_IMPLEMENTED" in str(e.value)
    with pytest.raises(wmb.WholeMemoryError) as e:
        g.multilayer_sample_begin(seeds, [30, 8193], random_seeds=[1, 2], weight_name="w")
    assert "NOT_IMPLEMENTED" in str(e.value)
    _destroy(ts + [wint, wshort])
