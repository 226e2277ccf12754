"""GraphSAGE neighbour aggregation on the MI355X (wholegraph_amd/torch/aggregation.py -> csrc/kernels/agg.hip).

Forward and backward are checked bit for bit against a numpy restatement of the order the header states
(include/wholememory/wholegraph_amd_ext.h, section 2b) and with allclose against torch autograd through an
index_select / index_add_ composite; then CuGraphSAGEConv against a hand-built Linear(cat(A, x_dst)), and a small
HomoGNNModel trained end to end on a planted-partition graph held in WholeMemory."""
import types

import numpy as np
import pytest

import _long_runs as LR

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---------------------------------------------------------------- the order, restated
def ref_forward(row_ptr, col, x, aggr):
    """out[d] = (S(d) [* fl(1/deg)], x[d]); S summed left to right from the first term; +0.0 for an empty target"""
    row_ptr = np.asarray(row_ptr, np.int64)
    n_dst, dim = len(row_ptr) - 1, x.shape[1]
    deg = np.diff(row_ptr)
    out = np.zeros((n_dst, 2 * dim), F32)
    acc = np.zeros((n_dst, dim), F32)
    for k in range(int(deg.max()) if n_dst else 0):   # k-th term of every target that has one: same order per target
        live = np.nonzero(deg > k)[0]
        term = x[col[row_ptr[live] + k]]
        acc[live] = term if k == 0 else acc[live] + term
    if aggr == "mean":
        nz = deg > 0
        acc[nz] = acc[nz] * (F32(1.0) / deg[nz].astype(F32))[:, None]
    acc[deg == 0] = F32(0.0)
    out[:, :dim] = acc
    out[:, dim:] = x[:n_dst]
    return out


def ref_backward(row_ptr, col, grad_out, n_src, aggr, chunk):
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, dim = len(row_ptr) - 1, grad_out.shape[1] // 2
    deg = np.diff(row_ptr)
    dst = np.repeat(np.arange(n_dst), deg)
    terms = grad_out[dst, :dim]
    if aggr == "mean":
        terms = terms * (F32(1.0) / deg[dst].astype(F32))[:, None]
    gx = np.zeros((n_src, dim), F32)
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(n_src + 1))
    for s in range(n_src):
        edges = order[starts[s]:starts[s + 1]]
        p = None
        for c0 in range(0, len(edges), chunk):
            part = terms[edges[c0]].copy()
            for e in edges[c0 + 1:c0 + chunk]:
                part = part + terms[e]
            p = part if p is None else p + part
        if s < n_dst:
            gx[s] = grad_out[s, dim:] if p is None else p + grad_out[s, dim:]
        elif p is not None:
            gx[s] = p
    return gx


def composite(x, row_ptr, col, aggr):
    """torch autograd reference: index_select + segment sum (index_add_), cat with the targets' rows"""
    import torch
    n_dst = row_ptr.numel() - 1
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=x.device), deg)
    agg = torch.zeros((n_dst, x.shape[1]), device=x.device, dtype=x.dtype).index_add_(0, dst, x.index_select(0, col.long()))
    if aggr == "mean":
        agg = agg / deg.clamp(min=1).to(x.dtype)[:, None]
    return torch.cat([agg, x[:n_dst]], dim=1)


def assert_close_sums(got, want, terms_abs, counts):
    """allclose (rtol 1e-5) with, per row, the worst-case error bound of a reordered fp32 sum of counts + 1 terms
    (|err| <= n u sum|t| for each of the two orders, u = 2^-24) as atol: rows of hubs sum thousands of terms, and the
    composite's index_add_ adds them in whatever order its atomics land"""
    import torch
    bound = 2.0 * (counts.double() + 1.0) * 2.0 ** -24 * terms_abs.double()
    diff = (got.double() - want.double()).abs()
    ok = diff <= 1e-5 * want.double().abs() + bound[:, None] + 1e-7
    assert bool(ok.all()), "max excess %g" % float((diff - bound[:, None]).max())


def abs_terms(row_ptr, col, g, n_src, aggr):
    """per source row: sum of |t(e)| over its edges + |self term| (the scale of its sum), and its edge count"""
    import torch
    n_dst, dim = row_ptr.numel() - 1, g.shape[1] // 2
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=g.device), deg)
    t = g[:, :dim].abs().index_select(0, dst)
    if aggr == "mean":
        t = t / deg.clamp(min=1).float()[dst][:, None]
    s = torch.zeros(n_src, device=g.device, dtype=torch.float64).index_add_(0, col.long(), t.double().max(1).values)
    s[:n_dst] += g[:, dim:].abs().max(1).values.double()
    counts = torch.bincount(col.long(), minlength=n_src)
    return s, counts


def block(rng, n_dst, n_src, max_deg, hub=None, hub_share=0.0, empty_every=7):
    deg = rng.integers(0, max_deg + 1, n_dst)
    deg[::empty_every] = 0
    if n_dst > 3:
        deg[1] = max_deg
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n_src, int(row_ptr[-1])).astype(np.int32)
    if hub is not None:
        col[rng.random(len(col)) < hub_share] = hub
    return row_ptr, col


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- 1 forward
@pytest.mark.parametrize("dim", [1, 3, 64, 127, 128, 256, 602])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_forward_bitwise(gpu_env, dim, aggr):
    from wholegraph_amd.torch.aggregation import agg_concat
    rng = np.random.default_rng(dim * 7 + len(aggr))
    n_dst, n_src = 301, 1000
    row_ptr, col = block(rng, n_dst, n_src, 64)
    x = rng.standard_normal((n_src, dim)).astype(F32)
    out = agg_concat(dev(x), dev(row_ptr), dev(col), aggr)
    assert out.shape == (n_dst, 2 * dim) and out.dtype.is_floating_point
    assert np.array_equal(bits(out), ref_forward(row_ptr, col, x, aggr).view(np.uint32))
    # int64 indices give the same result
    out64 = agg_concat(dev(x), dev(row_ptr.astype(np.int64)), dev(col.astype(np.int64)), aggr)
    assert np.array_equal(bits(out64), bits(out))


@pytest.mark.parametrize("dim", [3, 128])
def test_forward_strided_view_and_empty_blocks(gpu_env, dim):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    rng = np.random.default_rng(11)
    n_dst, n_src = 97, 400
    row_ptr, col = block(rng, n_dst, n_src, 40)
    wide = rng.standard_normal((n_src, dim + 9)).astype(F32)
    xv = dev(wide)[:, 4:4 + dim]   # row stride dim + 9, offset 4 floats: takes the element-wise path
    assert xv.stride(0) == dim + 9 and not xv.is_contiguous()
    for aggr in ("mean", "sum"):
        out = agg_concat(xv, dev(row_ptr), dev(col), aggr)
        assert np.array_equal(bits(out), ref_forward(row_ptr, col, wide[:, 4:4 + dim].copy(), aggr).view(np.uint32))
    x = dev(rng.standard_normal((n_src, dim)).astype(F32))
    # n_dst = 0
    out = agg_concat(x, dev(np.zeros(1, np.int32)), dev(np.zeros(0, np.int32)), "mean")
    assert out.shape == (0, 2 * dim)
    # E = 0: every target empty -> (+0.0, x[d])
    out = agg_concat(x, dev(np.zeros(6, np.int32)), dev(np.zeros(0, np.int32)), "mean")
    assert np.array_equal(bits(out[:, :dim]), np.zeros((5, dim), np.uint32))
    assert torch.equal(out[:, dim:], x[:5])


# ---------------------------------------------------------------- 2 backward
@pytest.mark.parametrize("dim", [1, 3, 64, 127, 128, 602])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_backward_bitwise_with_chunked_hub(gpu_env, dim, aggr):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat, chunk_edges
    C = chunk_edges()
    assert C >= 1
    rng = np.random.default_rng(100 + dim)
    n_dst, n_src = 300, 1200
    row_ptr, col = block(rng, n_dst, n_src, 64, hub=7, hub_share=0.45)
    col[rng.random(len(col)) < 0.1] = 950      # a second hub, not a target
    counts = np.bincount(col, minlength=n_src)
    assert counts[7] > 3 * C, "the chunked path and the chunk-order combine must run"
    assert (counts == 0).any() and (counts[:n_dst] == 0).any() and (counts[n_dst:] == 0).any()
    x_np = rng.standard_normal((n_src, dim)).astype(F32)
    g_np = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    g_np[5, dim:] = -0.0
    x = dev(x_np).requires_grad_(True)
    out = agg_concat(x, dev(row_ptr), dev(col), aggr)
    out.backward(dev(g_np))
    want = ref_backward(row_ptr, col, g_np, n_src, aggr, C)
    assert np.array_equal(bits(x.grad), want.view(np.uint32))
    # against torch autograd through the composite
    x2 = dev(x_np).requires_grad_(True)
    composite(x2, dev(row_ptr), dev(col), aggr).backward(dev(g_np))
    assert_close_sums(x.grad, x2.grad, *abs_terms(dev(row_ptr), dev(col), dev(g_np), n_src, aggr))
    # E = 0: grad_x = (G[s, F:2F] for s < n_dst, 0 after)
    x3 = dev(x_np).requires_grad_(True)
    agg_concat(x3, dev(np.zeros(n_dst + 1, np.int32)), dev(np.zeros(0, np.int32)), aggr).backward(dev(g_np))
    assert np.array_equal(bits(x3.grad[:n_dst]), g_np[:, dim:].view(np.uint32))
    assert not x3.grad[n_dst:].any()


@pytest.mark.parametrize("dim", [5, 8])
def test_backward_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, dim):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third"""
    from wholegraph_amd.torch.aggregation import agg_concat, chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(900 + dim)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    x_np = rng.standard_normal((LR.N_SRC, dim)).astype(F32)
    g_np = rng.standard_normal((LR.N_DST, 2 * dim)).astype(F32)
    for aggr in ("mean", "sum"):
        x = dev(x_np).requires_grad_(True)
        agg_concat(x, dev(row_ptr), dev(col), aggr).backward(dev(g_np))
        want = ref_backward(row_ptr, col, g_np, LR.N_SRC, aggr, C)
        assert np.array_equal(bits(x.grad), want.view(np.uint32))


# ---------------------------------------------------------------- 3 determinism
def test_backward_is_bitwise_reproducible_on_power_law_block(gpu_env):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    rng = np.random.default_rng(5)
    n_dst, n_src, fan, dim = 20000, 120000, 30, 128
    row_ptr = (np.arange(n_dst + 1) * fan).astype(np.int32)
    col = (np.minimum(rng.zipf(1.3, n_dst * fan), n_src) - 1).astype(np.int32)
    assert np.bincount(col).max() > 4000
    x = dev(rng.standard_normal((n_src, dim)).astype(F32)).requires_grad_(True)
    g = dev(rng.standard_normal((n_dst, 2 * dim)).astype(F32))
    rp, ci = dev(row_ptr), dev(col)
    grads = []
    for _ in range(2):
        x.grad = None
        agg_concat(x, rp, ci, "mean").backward(g)
        grads.append(x.grad.clone())
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    x2 = x.detach().clone().requires_grad_(True)
    composite(x2, rp, ci, "mean").backward(g)
    assert_close_sums(grads[0], x2.grad, *abs_terms(rp, ci, g, n_src, "mean"))


# ---------------------------------------------------------------- 4 real sampler output
def _wm_array(comm, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


def test_on_sampler_blocks(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from test_graph_oracle import make_csr
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.graph_ops import add_csr_self_loop
    n_nodes, dim = 20011, 64
    row_ptr, col = make_csr(n_nodes, 70, 41, np.int64, heavy=[(3, 4000), (4, 0)])
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    seeds = torch.from_numpy(np.random.default_rng(3).permutation(n_nodes)[:512].astype(np.int64)).cuda()
    seeds[:2] = torch.tensor([3, 4])
    target_gids, _, csr_row_ptr, csr_col_ind = g.multilayer_sample_without_replacement(seeds, [30, 30],
                                                                                       random_seeds=[7, 8])
    rng = np.random.default_rng(9)
    blocks = [(csr_row_ptr[i], csr_col_ind[i], target_gids[i].numel()) for i in range(2)]
    blocks.append(add_csr_self_loop(csr_row_ptr[1], csr_col_ind[1]) + (target_gids[1].numel(),))
    for rp, ci, n_src in blocks:
        assert rp.dtype == torch.int32 and ci.dtype == torch.int32
        x_np = rng.standard_normal((n_src, dim)).astype(F32)
        x = dev(x_np).requires_grad_(True)
        out = agg_concat(x, rp, ci, "mean")
        rp_np, ci_np = rp.cpu().numpy(), ci.cpu().numpy()
        assert np.array_equal(bits(out), ref_forward(rp_np, ci_np, x_np, "mean").view(np.uint32))
        g_np = rng.standard_normal(tuple(out.shape)).astype(F32)
        out.backward(dev(g_np))
        x2 = dev(x_np).requires_grad_(True)
        ref = composite(x2, rp, ci, "mean")
        assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
        ref.backward(dev(g_np))
        assert_close_sums(x.grad, x2.grad, *abs_terms(rp, ci, dev(g_np), n_src, "mean"))
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


# ---------------------------------------------------------------- 5 CuGraphSAGEConv
@pytest.mark.parametrize("root_weight,project,normalize", [(True, False, False), (False, False, False),
                                                           (True, True, False), (True, False, True),
                                                           (False, True, True)])
def test_sage_conv_matches_linear_of_concat(gpu_env, root_weight, project, normalize):
    import torch
    import torch.nn.functional as Fn
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout = 150, 700, 48, 24
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    layer = CuGraphSAGEConv(cin, cout, root_weight=root_weight, project=project, normalize=normalize).cuda()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, 20)
    assert out.shape == (n_dst, cout)
    h = layer.pre_lin(x).relu() if project else x
    cat = composite(h, rp, ci, "mean")
    want = layer.lin(cat if root_weight else cat[:, :cin])
    if normalize:
        want = Fn.normalize(want, p=2.0, dim=-1)
    assert torch.allclose(out, want, rtol=1e-5, atol=1e-5)
    out.square().sum().backward()
    params = dict(layer.named_parameters())
    assert "lin.weight" in params and (("pre_lin.weight" in params) == project)
    for name, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
    assert x.grad is not None and x.grad.abs().sum() > 0


def test_sage_conv_rejects_max_and_min(gpu_env):
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError):
            CuGraphSAGEConv(8, 4, aggr=aggr)
    with pytest.raises(ValueError):
        CuGraphSAGEConv(8, 4, aggr="median")


# ---------------------------------------------------------------- 6 end to end
def _planted_partition(n, k, rng, deg=12, p_in=0.9):
    comm_of = rng.integers(0, k, n)
    members = [np.nonzero(comm_of == c)[0] for c in range(k)]
    rows = []
    for v in range(n):
        same = rng.random(deg) < p_in
        nbr = np.where(same, rng.choice(members[comm_of[v]], deg), rng.integers(0, n, deg))
        rows.append(np.unique(nbr[nbr != v]))
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    return row_ptr, np.concatenate(rows).astype(np.int64), comm_of


def test_homo_gnn_model_trains_end_to_end(gpu_env):
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    torch.manual_seed(1)
    rng = np.random.default_rng(2)
    n, k, dim = 4000, 4, 32
    row_ptr, col, labels_np = _planted_partition(n, k, rng)
    centres = rng.standard_normal((k, dim)).astype(F32)
    feats = (0.5 * centres[labels_np] + rng.standard_normal((n, dim)).astype(F32)).astype(F32)
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [n, dim])
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(torch.from_numpy(feats).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "adam", {})
    torch.cuda.synchronize()
    before = emb.get_embedding_tensor().get_local_tensor()[0].clone()

    wgth.set_framework("cugraph")
    args = types.SimpleNamespace(model="sage", hiddensize=64, layernum=2, classnum=k, dropout=0.1, neighbors="10,10",
                                 inferencesample="10,10", heads=1)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    labels = torch.from_numpy(labels_np).cuda()
    losses = []
    model.train()
    for step in range(40):
        ids = torch.from_numpy(rng.choice(n, 256, replace=False).astype(np.int64)).cuda()
        logits = model(ids)
        assert logits.shape == (256, k)
        loss = Fn.cross_entropy(logits, labels[ids])
        opt.zero_grad()
        loss.backward()
        opt.step()
        wm_opt.step(0.01)
        losses.append(float(loss.detach()))
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    assert np.isfinite(losses).all()
    assert last < 0.6 * first, "loss %.3f -> %.3f" % (first, last)
    after = emb.get_embedding_tensor().get_local_tensor()[0]
    changed = (after != before).any(dim=1)
    assert changed.float().mean() > 0.2, "gradients did not reach the WholeMemory embedding"
    model.eval()
    with torch.no_grad():
        ids = torch.arange(0, n, 4, device="cuda")
        acc = (model(ids).argmax(1) == labels[ids]).float().mean()
    assert acc > 0.7
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
