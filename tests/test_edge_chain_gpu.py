"""Edge ids and edge attributes carried through the fused hop and the one-call chain (MI355X). Every comparison is on integers
or copied values, so every bar is bit-exact equality.
  1 the route the library already shipped — the one-hop sampler with edge output, hop by hop, plus append_unique — is the
    reference for the edge ids of the chain and of the fused hop; their other outputs equal the same calls without edge ids;
  2 the edge ids are checked against the graph alone: each leads from its block edge's centre to its source, lies in the
    centre's CSR row and is not repeated under one centre;
  3 attributes of every supported dtype on CONTINUOUS and CHUNKED tensors equal attr[edge id]; float16 and a DISTRIBUTED tensor
    take the gather fallback and give the same;
  4 GraphStructure.multilayer_sample_with_edge_attributes returns the same under WM_MULTILAYER_CHAIN=0 and under a memory
    budget that declines the chain, and wholememory_ext_edge_chain_calls tells the routes apart;
  5 the deferred form feeds a gather before the host has waited;
  6 one training step of EdgeWeightedSAGEConv gives the same loss bits from either route."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_NODES = 20011
HEAVY = [(3, 5000), (4, 0), (5, 1500), (6, 31), (7, 201), (8, 129), (9, 1), (10, 30), (11, 29), (12, 0)]
FANOUTS = ([30, 30], [5, 10, 15])
ATTRS = {"w": np.float32, "i32": np.int32, "i64": np.int64, "f64": np.float64}


def _wm_array(comm, mt, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, mt, "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


def _graph(comm, id_dtype, mt="chunked", extra=False):
    """degrees uniform in [0, 60] — below and above every fan-out of the tests — with hubs, nodes without edges and degrees
    next to the fan-outs at fixed nodes; one edge attribute per supported dtype (`w` also serves as the sampling weight)"""
    import wholegraph_amd.torch as wgth
    from test_graph_oracle import make_csr
    row_ptr, col = make_csr(N_NODES, 60, 7, id_dtype, heavy=HEAVY)
    rng = np.random.default_rng(23)
    n_edges = col.shape[0]
    host = {"w": np.power(10.0, rng.uniform(-3.0, 3.0, n_edges)).astype(np.float32),
            "i32": rng.integers(-(1 << 31), 1 << 31, n_edges).astype(np.int32),
            "i64": rng.integers(-(1 << 62), 1 << 62, n_edges).astype(np.int64),
            "f64": rng.standard_normal(n_edges)}
    host["w"][::5] = 2.0
    ts = {"row": _wm_array(comm, mt, row_ptr), "col": _wm_array(comm, mt, col)}
    g = wgth.GraphStructure()
    g.set_csr_graph(ts["row"], ts["col"])
    for name, arr in host.items():
        assert arr.dtype == ATTRS[name]
        ts[name] = _wm_array(comm, mt, arr)
        g.set_edge_attribute(name, ts[name])
    if extra:       # what the attribute kernel does not take
        host["f16"] = rng.standard_normal(n_edges).astype(np.float16)
        host["dist"] = rng.standard_normal(n_edges).astype(np.float32)
        ts["f16"] = _wm_array(comm, mt, host["f16"])
        ts["dist"] = _wm_array(comm, "distributed", host["dist"])
        g.set_edge_attribute("f16", ts["f16"])
        g.set_edge_attribute("dist", ts["dist"])
    return g, ts, row_ptr, col, host


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts.values():
        wgth.destroy_wholememory_tensor(t)


def _seeds(id_dtype):
    import torch
    picked = np.random.default_rng(9).permutation(N_NODES)[:300]
    return torch.from_numpy(np.concatenate([[n for n, _ in HEAVY], [7, 3], picked]).astype(id_dtype)).cuda()


def _calls():
    from wholegraph_amd import binding
    return binding.lib().wholememory_ext_edge_chain_calls()


def _assert_lists_equal(got, ref, what=""):
    import torch
    assert len(got) == len(ref), what
    for k, (a_list, b_list) in enumerate(zip(got, ref)):
        assert len(a_list) == len(b_list), (what, k)
        for layer, (a, b) in enumerate(zip(a_list, b_list)):
            if isinstance(a, dict):
                assert list(a) == list(b), (what, layer)
                for name in a:
                    assert a[name].dtype == b[name].dtype and tuple(a[name].shape) == tuple(b[name].shape), (what, layer, name)
                    assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), (what, layer, name)
            else:
                assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, k, layer, a.shape, b.shape)
                assert torch.equal(a, b), (what, k, layer)


def _reference_hops(g, seeds, fanouts, weight_name, hop_seeds):
    """per hop (offsets, unique, neighbor_pos, center_lid, edge ids) over the one-hop sampler with edge output + append_unique"""
    import wholegraph_amd.torch.graph_ops as gops
    out, frontier = [], seeds
    for depth, fanout in enumerate(fanouts):
        if weight_name is None:
            off, ids, lid, eid = g.unweighted_sample_without_replacement_one_hop(
                frontier, fanout, random_seed=hop_seeds[depth], need_center_local_output=True, need_edge_output=True)
        else:
            off, ids, lid, eid = g.weighted_sample_without_replacement_one_hop(
                weight_name, frontier, fanout, random_seed=hop_seeds[depth], need_center_local_output=True, need_edge_output=True)
        uniq, pos = gops.append_unique(frontier, ids, need_neighbor_raw_to_unique=True)
        out.append((off, uniq, pos, lid, eid))
        frontier = uniq
    return out


CASES = [(idt, wn, fan) for idt in (np.int32, np.int64) for wn in (None, "w") for fan in FANOUTS]


@pytest.mark.parametrize("id_dtype,weight_name,fanouts", CASES)
def test_edge_ids_equal_the_one_hop_sampler_and_the_graph(gpu_env, id_dtype, weight_name, fanouts):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    g, ts, row_ptr, col, host = _graph(gpu_env, id_dtype)
    csr = (ts["row"].wmb_tensor, ts["col"].wmb_tensor)
    wgt = None if weight_name is None else ts[weight_name].wmb_tensor
    seeds, hop_seeds = _seeds(id_dtype), [77 + 5 * i for i in range(len(fanouts))]
    ref = _reference_hops(g, seeds, fanouts, weight_name, hop_seeds)
    for depth in range(len(fanouts)):     # the reference itself covers what the issue asks of the graph
        deg = np.diff(ref[depth][0].cpu().numpy())
        assert (deg == fanouts[depth]).any() and (deg == 0).any() and ((deg > 0) & (deg < fanouts[depth])).any()

    # -- 1a the chain with edge ids
    before = _calls()
    chain = wops.multilayer_sample(*csr, seeds, fanouts, hop_seeds, wm_csr_weight_ptr_tensor=wgt, need_edge_ids=True)
    assert chain is not None and _calls() == before + 1
    plain = wops.multilayer_sample(*csr, seeds, fanouts, hop_seeds, wm_csr_weight_ptr_tensor=wgt)
    assert plain is not None and _calls() == before + 1
    assert [len(hop) for hop in chain] == [6] * len(fanouts) and [len(hop) for hop in plain] == [5] * len(fanouts)
    for depth, (hop, hop_plain, hop_ref) in enumerate(zip(chain, plain, ref)):
        for k, name in enumerate(("offsets", "unique", "neighbor_pos", "center_lid")):
            assert hop[k].dtype == hop_plain[k].dtype and torch.equal(hop[k], hop_plain[k]), (name, depth)
            assert hop[k].dtype == hop_ref[k].dtype and torch.equal(hop[k], hop_ref[k]), (name, depth)
        assert torch.equal(hop[4], hop_plain[4]), depth
        assert hop[5].dtype == torch.int64 and torch.equal(hop[5], hop_ref[4]), "edge ids of the chain differ at hop %d" % depth

    # -- 1b the fused hop with edge ids, hop by hop
    frontier = seeds
    for depth, fanout in enumerate(fanouts):
        fused = wops.sample_append_unique(*csr, frontier, fanout, hop_seeds[depth], wm_csr_weight_ptr_tensor=wgt,
                                          need_edge_output=True)
        fused_plain = wops.sample_append_unique(*csr, frontier, fanout, hop_seeds[depth], wm_csr_weight_ptr_tensor=wgt)
        assert fused is not None and len(fused) == 5 and len(fused_plain) == 4
        for k, name in enumerate(("offsets", "unique", "neighbor_pos", "center_lid")):
            assert fused[k].dtype == fused_plain[k].dtype and torch.equal(fused[k], fused_plain[k]), (name, depth)
            assert torch.equal(fused[k], ref[depth][k]), (name, depth)
        assert fused[4].dtype == torch.int64 and torch.equal(fused[4], ref[depth][4]), "edge ids of the fused hop differ at hop %d" % depth
        frontier = fused[1]

    # -- 2 against the graph alone, through the public sampler (layers outermost first)
    gids, _, rps, cis, attrs = g.multilayer_sample_with_edge_attributes(seeds, fanouts, ["__edge_id__"], weight_name,
                                                                       random_seeds=hop_seeds)
    assert _calls() == before + 2
    for layer in range(len(fanouts)):
        eid = attrs[layer]["__edge_id__"].cpu().numpy()
        target = gids[layer].cpu().numpy().astype(np.int64)
        rp = rps[layer].cpu().numpy().astype(np.int64)
        ci = cis[layer].cpu().numpy()
        assert eid.dtype == np.int64 and eid.shape == ci.shape
        assert np.array_equal(eid, chain[len(fanouts) - 1 - layer][5].cpu().numpy())
        assert np.array_equal(col[eid].astype(np.int64), target[ci]), "graph_col_ind[eid] != target_gids[csr_col_ind]"
        centre_pos = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        centre = target[centre_pos]
        assert np.all((row_ptr[centre] <= eid) & (eid < row_ptr[centre + 1])), "edge id outside its centre's CSR row"
        pairs = np.stack([centre_pos, eid], axis=1)
        assert np.unique(pairs, axis=0).shape[0] == pairs.shape[0], "an edge id is repeated under one centre"
    _destroy(ts)


@pytest.mark.parametrize("mt", ["continuous", "chunked"])
@pytest.mark.parametrize("id_dtype,weight_name,fanouts", [(np.int32, "w", [30, 30]), (np.int64, None, [5, 10, 15])])
def test_attributes_equal_the_attribute_at_the_edge_id(gpu_env, mt, id_dtype, weight_name, fanouts):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    g, ts, row_ptr, col, host = _graph(gpu_env, id_dtype, mt, extra=True)
    csr = (ts["row"].wmb_tensor, ts["col"].wmb_tensor)
    wgt = None if weight_name is None else ts[weight_name].wmb_tensor
    seeds, hop_seeds = _seeds(id_dtype), [5 + 3 * i for i in range(len(fanouts))]
    # the op itself: the kernel fills every supported dtype, in the order given
    order = ["f64", "w", "i64", "i32"]
    before = _calls()
    chain = wops.multilayer_sample(*csr, seeds, fanouts, hop_seeds, wm_csr_weight_ptr_tensor=wgt,
                                   wm_edge_attr_tensors=[ts[n] for n in order])
    assert chain is not None and _calls() == before + 1
    for hop in chain:
        assert len(hop) == 7 and len(hop[6]) == len(order)
        eid = hop[5].cpu().numpy()
        assert eid.shape[0] > 0
        for name, got in zip(order, hop[6]):
            got = got.cpu().numpy()
            assert got.dtype == ATTRS[name] and got.shape == eid.shape
            assert got.tobytes() == host[name][eid].tobytes(), "%s (%s) differs" % (name, mt)
    # nine attributes: two launches per hop
    nine = (order * 3)[:9]
    many = wops.multilayer_sample(*csr, seeds, fanouts, hop_seeds, wm_csr_weight_ptr_tensor=wgt,
                                  wm_edge_attr_tensors=[ts[n] for n in nine])
    assert many is not None
    for hop, hop4 in zip(many, chain):
        assert torch.equal(hop[5], hop4[5])
        for name, got in zip(nine, hop[6]):
            assert got.cpu().numpy().tobytes() == host[name][hop[5].cpu().numpy()].tobytes(), name
    # what the kernel does not take is declined by the op ...
    for bad in ("f16", "dist"):
        assert wops.multilayer_sample(*csr, seeds, fanouts, hop_seeds, wm_csr_weight_ptr_tensor=wgt,
                                      wm_edge_attr_tensors=[ts["w"], ts[bad]]) is None, bad
    # ... and fetched by the gather fallback of the public sampler, which stays on the chain for the rest
    names = ["f16", "i64", "dist", "__edge_id__", "w", "f64", "i32"]
    before = _calls()
    got = g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    assert _calls() == before + 1
    for layer in range(len(fanouts)):
        assert list(got[4][layer]) == names
        eid = got[4][layer]["__edge_id__"].cpu().numpy()
        assert np.array_equal(eid, chain[len(fanouts) - 1 - layer][5].cpu().numpy())
        for name in names:
            if name != "__edge_id__":
                v = got[4][layer][name].cpu().numpy()
                assert v.dtype == host[name].dtype and v.tobytes() == host[name][eid].tobytes(), "%s (%s) differs" % (name, mt)
    _destroy(ts)


@pytest.mark.parametrize("id_dtype,weight_name,fanouts", CASES)
def test_public_sampler_is_the_same_on_every_route(gpu_env, knobs, id_dtype, weight_name, fanouts):
    g, ts, row_ptr, col, host = _graph(gpu_env, id_dtype)
    seeds, hop_seeds = _seeds(id_dtype), [1000 + i for i in range(len(fanouts))]
    names = ["w", "i64", "__edge_id__", "i32", "f64"]
    before = _calls()
    got = g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    assert _calls() == before + 1
    again = g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    assert _calls() == before + 2
    _assert_lists_equal(again, got, "second call")
    plain = g.multilayer_sample_without_replacement(seeds, fanouts, weight_name, random_seeds=hop_seeds)
    _assert_lists_equal(got[:4], plain, "four lists")
    knobs.set("WM_MULTILAYER_CHAIN", "0")
    hop_by_hop = g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    assert _calls() == before + 2, "the chain ran although WM_MULTILAYER_CHAIN=0"
    knobs.unset("WM_MULTILAYER_CHAIN")
    _assert_lists_equal(got, hop_by_hop, "WM_MULTILAYER_CHAIN=0")
    knobs.set("WM_MULTILAYER_MAX_BYTES", "1")
    declined = g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    assert _calls() == before + 2, "the chain ran beyond its memory budget"
    knobs.unset("WM_MULTILAYER_MAX_BYTES")
    _assert_lists_equal(got, declined, "WM_MULTILAYER_MAX_BYTES=1")
    g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    assert _calls() == before + 3
    _destroy(ts)


def test_seeds_are_drawn_one_per_hop_in_hop_order(gpu_env, knobs):
    import random
    g, ts, row_ptr, col, host = _graph(gpu_env, np.int64)
    seeds, fanouts = _seeds(np.int64), [5, 10, 15]
    r = random.Random(12345)
    drawn = [r.getrandbits(64) for _ in fanouts]
    fourth = r.getrandbits(64)
    ref = g.multilayer_sample_with_edge_attributes(seeds, fanouts, ["w", "__edge_id__"], "w", random_seeds=drawn)
    for chain in ("1", "0"):
        knobs.set("WM_MULTILAYER_CHAIN", chain)
        random.seed(12345)
        got = g.multilayer_sample_with_edge_attributes(seeds, fanouts, ["w", "__edge_id__"], "w")
        _assert_lists_equal(got, ref, "WM_MULTILAYER_CHAIN=" + chain)
        assert random.getrandbits(64) == fourth, "not exactly one draw per hop"
    _destroy(ts)


@pytest.mark.parametrize("id_dtype,weight_name,fanouts", [(np.int32, "w", [30, 30]), (np.int64, None, [5, 10, 15])])
def test_deferred_form_feeds_the_gather(gpu_env, id_dtype, weight_name, fanouts):
    import torch
    import wholegraph_amd.torch as wgth
    dim = 32
    g, ts, row_ptr, col, host = _graph(gpu_env, id_dtype, extra=True)
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [N_NODES, dim])
    local, _ = emb.get_embedding_tensor().get_local_tensor()
    local.copy_(torch.arange(N_NODES, device="cuda", dtype=torch.float32).unsqueeze(1) + torch.arange(dim, device="cuda") / 64.0)
    seeds, hop_seeds = _seeds(id_dtype), [11 + 3 * i for i in range(len(fanouts))]
    names = ["w", "__edge_id__", "f16", "i64"]
    ref = g.multilayer_sample_with_edge_attributes(seeds, fanouts, names, weight_name, random_seeds=hop_seeds)
    before = _calls()
    h = g.multilayer_sample_begin(seeds, fanouts, random_seeds=hop_seeds, weight_name=weight_name, edge_attr_names=names)
    assert _calls() == before + 1
    padded = h.padded_frontier
    out = torch.full((padded.shape[0], dim), -7.0, device="cuda")
    emb.gather(padded, out=out)                      # queued behind the sampling kernels, before result()
    got = h.result()
    torch.cuda.synchronize()
    assert len(got) == 5
    _assert_lists_equal(got, ref, "deferred")
    n = got[0][0].shape[0]
    assert padded.shape[0] > n                       # the chain handed out its upper-bound array
    assert torch.equal(padded[:n], got[0][0]) and bool((padded[n:] == -1).all())
    assert torch.equal(out[:n], emb.gather(got[0][0])) and bool((out[n:] == -7.0).all())
    # without names the handle returns the four lists as before
    four = g.multilayer_sample_begin(seeds, fanouts, random_seeds=hop_seeds, weight_name=weight_name).result()
    assert len(four) == 4
    _assert_lists_equal(four, ref[:4], "deferred, no names")
    wgth.destroy_embedding(emb)
    _destroy(ts)


def test_training_step_gives_the_same_loss_bits_from_either_route(gpu_env, knobs):
    import torch
    import torch.nn.functional as Fn
    from wholegraph_amd.torch.cugraphops import EdgeWeightedSAGEConv
    g, ts, row_ptr, col, host = _graph(gpu_env, np.int64)
    rng = np.random.default_rng(9)
    feats = torch.from_numpy(rng.standard_normal((N_NODES, 16)).astype(np.float32)).cuda()
    labels = torch.from_numpy(rng.integers(0, 4, N_NODES).astype(np.int64)).cuda()
    ids = torch.from_numpy(rng.choice(N_NODES, 128, replace=False).astype(np.int64)).cuda()

    def step():
        torch.manual_seed(1)
        l1, l2 = EdgeWeightedSAGEConv(16, 32).cuda(), EdgeWeightedSAGEConv(32, 4).cuda()
        gids, _, rps, cis, attrs = g.multilayer_sample_with_edge_attributes(ids, [8, 8], ["w"], "w", random_seeds=[100, 200])
        w0, w1 = attrs[0]["w"].clone().requires_grad_(True), attrs[1]["w"].clone().requires_grad_(True)
        h = l1(feats[gids[0]], rps[0], cis[0], 8, w0).relu()
        loss = Fn.cross_entropy(l2(h, rps[1], cis[1], 8, w1), labels[ids])
        loss.backward()
        return loss.detach(), w0.grad, w1.grad, l1.lin.weight.grad

    before = _calls()
    new = step()
    assert _calls() == before + 1
    knobs.set("WM_MULTILAYER_CHAIN", "0")
    old = step()
    assert _calls() == before + 1
    assert torch.isfinite(new[0])
    for a, b in zip(new, old):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    _destroy(ts)
