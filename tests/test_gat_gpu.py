"""GAT attention aggregation on the MI355X (wholegraph_amd/torch/gat_aggregation.py -> csrc/kernels/gat.hip).

alpha is checked against a float64 softmax; every other output bit for bit against a numpy restatement of the order the
header states (include/wholememory/wholegraph_amd_ext.h, section 2c), fed the op's own alpha, and with allclose against
torch autograd through an index_select / scatter-max / index_add_ composite. Then CuGraphGATConv against the composite,
and a two-layer GAT trained end to end on a planted-partition graph held in WholeMemory."""
import numpy as np
import pytest

import _long_runs as LR
from test_sage_agg_gpu import _planted_partition, _wm_array, bits, block, dev

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24


# ---------------------------------------------------------------- the order, restated
def ref_scores(h, att, H, n_dst):
    """(s_src [n_src, H], s_dst [n_dst, H]): att[half, k, :] . h[j, k, :], left to right over f"""
    n_src, hf = h.shape
    F = hf // H
    hv, a = h.reshape(n_src, H, F), att.reshape(2, H, F)
    s_src = np.full((n_src, H), -0.0, F32)
    s_dst = np.full((n_dst, H), -0.0, F32)
    for f in range(F):
        s_src = s_src + a[0, :, f] * hv[:, :, f]
        s_dst = s_dst + a[1, :, f] * hv[:n_dst, :, f]
    return s_src, s_dst


def edge_dst(row_ptr):
    row_ptr = np.asarray(row_ptr, np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def seg_sum(row_ptr, terms):
    """per target, the sum of its edges' terms left to right from the first; +0.0 for a target without edges"""
    row_ptr = np.asarray(row_ptr, np.int64)
    deg = np.diff(row_ptr)
    acc = np.full((len(deg),) + terms.shape[1:], -0.0, F32)
    for k in range(int(deg.max()) if len(deg) else 0):
        live = np.nonzero(deg > k)[0]
        acc[live] = acc[live] + terms[row_ptr[live] + k]
    acc[deg == 0] = F32(0.0)
    return acc


def ref_out(row_ptr, col, h, alpha, H, concat):
    n_dst = len(row_ptr) - 1
    F = h.shape[1] // H
    terms = alpha[:, :, None] * h[np.asarray(col, np.int64)].reshape(-1, H, F)
    o = seg_sum(row_ptr, terms)
    if concat:
        return o.reshape(n_dst, H * F)
    acc = o[:, 0]
    for k in range(1, H):
        acc = acc + o[:, k]
    return acc * (F32(1.0) / F32(H))


def ref_alpha64(row_ptr, col, h, att, H, slope):
    """float64 softmax over each target's edges of the fp32 logits l (restated bit for bit), and per edge a bound of a few
    fp32 ulp plus the rounding of den (deg terms) and of l - max"""
    s_src, s_dst = ref_scores(h, att, H, len(row_ptr) - 1)
    dst = edge_dst(row_ptr)
    z = s_src[np.asarray(col, np.int64)] + s_dst[dst]
    l = np.where(z > 0, z, F32(slope) * z).astype(np.float64)
    m = np.full((len(row_ptr) - 1, H), -np.inf)
    np.maximum.at(m, dst, l)
    w = np.exp(l - m[dst])
    den = np.zeros_like(m)
    np.add.at(den, dst, w)
    ref = w / den[dst]
    deg = np.diff(np.asarray(row_ptr, np.int64))[dst][:, None]
    spread = np.zeros_like(m)   # per target: the largest |l - max| (the rounding of l - max enters every w of den)
    np.maximum.at(spread, dst, np.abs(l - m[dst]))
    bound = (8.0 + deg + spread[dst]) * 2 * U * ref + 1e-38
    return ref, bound


def ref_backward(row_ptr, col, h, att, alpha, G, H, slope, concat, chunk, node_chunk):
    """(grad_h, grad_att) in the stated order, from the op's alpha"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, n_src, hf = len(row_ptr) - 1, h.shape[0], h.shape[1]
    F = hf // H
    hv, a = h.reshape(n_src, H, F), att.reshape(2, H, F)
    Gk = G.reshape(n_dst, H, F) if concat else G[:, None, :] * (F32(1.0) / F32(H))
    dst = edge_dst(row_ptr)
    E = len(col)
    s_src, s_dst = ref_scores(h, att, H, n_dst)
    da = np.full((E, H), -0.0, F32)
    for f in range(F):
        da = da + Gk[dst, :, f] * hv[col, :, f]
    c = seg_sum(row_ptr, alpha * da)
    z = s_src[col] + s_dst[dst]
    dl = alpha * (da - c[dst])
    dz = np.where(z > 0, dl, dl * F32(slope)).astype(F32)
    ds_dst = seg_sum(row_ptr, dz)
    tP = alpha[:, :, None] * Gk[dst]
    P = np.zeros((n_src, H, F), F32)
    ds_src = np.zeros((n_src, H), F32)
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(n_src + 1))
    for j in range(n_src):
        edges = order[starts[j]:starts[j + 1]]
        if len(edges) == 0:
            continue
        p = q = None
        for c0 in range(0, len(edges), chunk):
            pp, qq = tP[edges[c0]].copy(), dz[edges[c0]].copy()
            for e in edges[c0 + 1:c0 + chunk]:
                pp, qq = pp + tP[e], qq + dz[e]
            p, q = (pp, qq) if p is None else (p + pp, q + qq)
        P[j], ds_src[j] = p, q
    gh = P + ds_src[:, :, None] * a[0]
    gh[:n_dst] = gh[:n_dst] + ds_dst[:, :, None] * a[1]
    ga = np.zeros((2, H, F), F32)
    for half, ds, rows in ((0, ds_src, n_src), (1, ds_dst, n_dst)):
        if rows == 0:
            continue
        tot = np.full((H, F), -0.0, F32)
        for q0 in range(0, rows, node_chunk):
            part = np.full((H, F), -0.0, F32)
            for j in range(q0, min(rows, q0 + node_chunk)):
                part = part + ds[j][:, None] * hv[j]
            tot = tot + part
        ga[half] = tot
    return gh.reshape(n_src, hf), ga.reshape(-1)


def composite(h, att, row_ptr, col, H, slope, concat):
    """torch autograd reference: index_select, a scatter-max / exp / index_add_ softmax, index_add_"""
    import torch
    n_dst = row_ptr.numel() - 1
    F = h.shape[1] // H
    hv, a = h.view(-1, H, F), att.view(2, H, F)
    s_src = (hv * a[0]).sum(-1)
    s_dst = (hv[:n_dst] * a[1]).sum(-1)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=h.device), deg)
    col = col.long()
    l = torch.nn.functional.leaky_relu(s_src[col] + s_dst[dst], slope)
    m = torch.full((n_dst, H), -float("inf"), device=h.device).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=h.device).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=h.device).index_add_(0, dst, alpha[:, :, None] * hv[col])
    return o.reshape(n_dst, H * F) if concat else o.mean(1)


def assert_close_scaled(got, want, rtol=1e-4):
    """allclose with an absolute part scaled to the tensor (hub rows sum thousands of terms; the composite's index_add_
    adds them in whatever order its atomics land)"""
    import torch
    got, want = got.double(), want.double()
    tol = rtol * want.abs() + rtol * float(want.abs().max()) + 1e-7
    diff = (got - want).abs()
    assert bool((diff <= tol).all()), "max excess %g" % float((diff - tol).max())


def inputs(rng, n_src, H, F, scale=0.5):
    h = rng.standard_normal((n_src, H * F)).astype(F32)
    att = (scale * rng.standard_normal(2 * H * F) / np.sqrt(F)).astype(F32)
    return h, att


# ---------------------------------------------------------------- 1 forward
@pytest.mark.parametrize("H", [1, 2, 4, 8])
@pytest.mark.parametrize("F", [1, 3, 16, 64, 127])
def test_forward_alpha_and_out(gpu_env, H, F):
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    rng = np.random.default_rng(H * 131 + F)
    n_dst, n_src = 157, 600
    row_ptr, col = block(rng, n_dst, n_src, 40)
    h, att = inputs(rng, n_src, H, F)
    for concat in (True, False):
        out, alpha = mha_gat_n2n(dev(h), dev(att), dev(row_ptr), dev(col), H, 0.2, concat, return_alpha=True)
        assert out.shape == ((n_dst, H * F) if concat else (n_dst, F)) and alpha.shape == (len(col), H)
        al = alpha.cpu().numpy()
        ref, bound = ref_alpha64(row_ptr, col, h, att, H, 0.2)
        assert (np.abs(al - ref) <= bound).all(), "alpha off by %g" % float(np.max(np.abs(al - ref) / (ref + 1e-30)))
        assert np.array_equal(bits(out), ref_out(row_ptr, col, h, al, H, concat).view(np.uint32))
        out64 = mha_gat_n2n(dev(h), dev(att), dev(row_ptr.astype(np.int64)), dev(col.astype(np.int64)), H, 0.2, concat)
        assert np.array_equal(bits(out64), bits(out))


@pytest.mark.parametrize("F", [3, 32])
def test_forward_strided_and_empty_blocks(gpu_env, F):
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    rng = np.random.default_rng(17 + F)
    H, n_dst, n_src = 4, 97, 400
    row_ptr, col = block(rng, n_dst, n_src, 30)
    wide = rng.standard_normal((n_src, H * F + 9)).astype(F32)
    _, att = inputs(rng, n_src, H, F)
    hv = dev(wide)[:, 4:4 + H * F]   # row stride H*F + 9, offset 4 floats: the element-wise path
    assert not hv.is_contiguous()
    h = wide[:, 4:4 + H * F].copy()
    for concat in (True, False):
        out, alpha = mha_gat_n2n(hv, dev(att), dev(row_ptr), dev(col), H, 0.2, concat, return_alpha=True)
        al = alpha.cpu().numpy()
        ref, bound = ref_alpha64(row_ptr, col, h, att, H, 0.2)
        assert (np.abs(al - ref) <= bound).all()
        assert np.array_equal(bits(out), ref_out(row_ptr, col, h, al, H, concat).view(np.uint32))
    x = dev(h)
    out = mha_gat_n2n(x, dev(att), dev(np.zeros(1, np.int32)), dev(np.zeros(0, np.int32)), H)   # n_dst = 0
    assert out.shape == (0, H * F)
    out, alpha = mha_gat_n2n(x, dev(att), dev(np.zeros(6, np.int32)), dev(np.zeros(0, np.int32)), H, concat=False,
                             return_alpha=True)   # E = 0: every target +0.0
    assert out.shape == (5, F) and alpha.shape == (0, H)
    assert np.array_equal(bits(out), np.zeros((5, F), np.uint32))


# ---------------------------------------------------------------- 2 backward
@pytest.mark.parametrize("H,F", [(1, 3), (2, 16), (4, 32), (8, 1), (4, 127)])
@pytest.mark.parametrize("concat", [True, False])
def test_backward_bitwise_with_chunked_hub(gpu_env, H, F, concat):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    C, N = chunk_edges(), node_chunk()
    rng = np.random.default_rng(300 + 10 * H + F + concat)
    n_dst, n_src = 400, N + N // 2 + 17    # grad_att: two node chunks, the second partial
    row_ptr, col = block(rng, n_dst, n_src, 48, hub=7, hub_share=0.3)
    col[rng.random(len(col)) < 0.05] = n_src - 3   # a second hub, not a target
    counts = np.bincount(col, minlength=n_src)
    assert counts[7] > 3 * C, "the chunked path and the chunk-order combine must run"
    assert (counts == 0).any() and (counts[:n_dst] == 0).any()
    h_np, att_np = inputs(rng, n_src, H, F)
    G_np = rng.standard_normal((n_dst, H * F if concat else F)).astype(F32)
    h = dev(h_np).requires_grad_(True)
    att = dev(att_np).requires_grad_(True)
    out, alpha = mha_gat_n2n(h, att, dev(row_ptr), dev(col), H, 0.2, concat, return_alpha=True)
    out.backward(dev(G_np))
    gh, ga = ref_backward(row_ptr, col, h_np, att_np, alpha.cpu().numpy(), G_np, H, 0.2, concat, C, N)
    assert np.array_equal(bits(h.grad), gh.view(np.uint32))
    assert np.array_equal(bits(att.grad), ga.view(np.uint32))
    # against torch autograd through the composite
    h2 = dev(h_np).requires_grad_(True)
    att2 = dev(att_np).requires_grad_(True)
    want = composite(h2, att2, dev(row_ptr), dev(col), H, 0.2, concat)
    assert_close_scaled(out.detach(), want.detach(), 1e-5)
    want.backward(dev(G_np))
    assert_close_scaled(h.grad, h2.grad)
    assert_close_scaled(att.grad, att2.grad)


@pytest.mark.parametrize("F", [5, 8])
def test_backward_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, F):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third,
    each with the chunk's ds_src loaded next to the row"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    C, N, H = chunk_edges(), node_chunk(), 2
    rng = np.random.default_rng(900 + F)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    h_np, att_np = inputs(rng, LR.N_SRC, H, F)
    for concat in (True, False):
        G_np = rng.standard_normal((LR.N_DST, H * F if concat else F)).astype(F32)
        h = dev(h_np).requires_grad_(True)
        att = dev(att_np).requires_grad_(True)
        out, alpha = mha_gat_n2n(h, att, dev(row_ptr), dev(col), H, 0.2, concat, return_alpha=True)
        out.backward(dev(G_np))
        gh, ga = ref_backward(row_ptr, col, h_np, att_np, alpha.cpu().numpy(), G_np, H, 0.2, concat, C, N)
        assert np.array_equal(bits(h.grad), gh.view(np.uint32))
        assert np.array_equal(bits(att.grad), ga.view(np.uint32))


def test_backward_empty_blocks(gpu_env):
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    rng = np.random.default_rng(8)
    H, F, n_src = 2, 8, 50
    h_np, att_np = inputs(rng, n_src, H, F)
    for n_dst in (0, 6):   # n_dst = 0, then E = 0 with targets
        G_np = rng.standard_normal((n_dst, H * F)).astype(F32)
        h = dev(h_np).requires_grad_(True)
        att = dev(att_np).requires_grad_(True)
        rp = np.zeros(n_dst + 1, np.int32)
        out = mha_gat_n2n(h, att, dev(rp), dev(np.zeros(0, np.int32)), H)
        out.backward(dev(G_np))
        gh, ga = ref_backward(rp, np.zeros(0, np.int32), h_np, att_np, np.zeros((0, H), F32), G_np, H, 0.2, True,
                              chunk_edges(), node_chunk())
        assert np.array_equal(bits(h.grad), gh.view(np.uint32)) and not h.grad.any()
        assert np.array_equal(bits(att.grad), ga.view(np.uint32))


# ---------------------------------------------------------------- 3 stability
def test_large_logits_stay_finite(gpu_env):
    import torch
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    rng = np.random.default_rng(4)
    H, F, n_dst, n_src = 4, 16, 200, 800
    row_ptr, col = block(rng, n_dst, n_src, 30)
    h_np = rng.standard_normal((n_src, H * F)).astype(F32)
    att_np = (250.0 * rng.standard_normal(2 * H * F)).astype(F32)   # scores of order 1e3
    s_src, _ = ref_scores(h_np, att_np, H, n_dst)
    assert np.abs(s_src).max() > 1e3
    h = dev(h_np).requires_grad_(True)
    att = dev(att_np).requires_grad_(True)
    out, alpha = mha_gat_n2n(h, att, dev(row_ptr), dev(col), H, 0.2, True, return_alpha=True)
    assert torch.isfinite(out).all() and torch.isfinite(alpha).all()
    deg = np.diff(row_ptr)
    sums = np.add.reduceat(alpha.cpu().numpy(), row_ptr[:-1][deg > 0], axis=0) if (deg > 0).any() else None
    assert np.allclose(sums, 1.0, atol=1e-5)
    out.square().sum().backward()
    assert torch.isfinite(h.grad).all() and torch.isfinite(att.grad).all()


# ---------------------------------------------------------------- 4 reproducibility
def test_backward_is_bitwise_reproducible_on_power_law_block(gpu_env):
    import torch
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    rng = np.random.default_rng(5)
    n_dst, n_src, fan, H, F = 20000, 120000, 30, 4, 32
    row_ptr = (np.arange(n_dst + 1) * fan).astype(np.int32)
    col = (np.minimum(rng.zipf(1.3, n_dst * fan), n_src) - 1).astype(np.int32)
    assert np.bincount(col).max() > 4000
    h_np, att_np = inputs(rng, n_src, H, F)
    h = dev(h_np).requires_grad_(True)
    att = dev(att_np).requires_grad_(True)
    G = dev(rng.standard_normal((n_dst, H * F)).astype(F32))
    rp, ci = dev(row_ptr), dev(col)
    grads = []
    for _ in range(2):
        h.grad = att.grad = None
        mha_gat_n2n(h, att, rp, ci, H).backward(G)
        grads.append((h.grad.clone(), att.grad.clone()))
    for a, b in zip(*grads):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    h2 = dev(h_np).requires_grad_(True)
    att2 = dev(att_np).requires_grad_(True)
    composite(h2, att2, rp, ci, H, 0.2, True).backward(G)
    assert_close_scaled(grads[0][0], h2.grad)
    assert_close_scaled(grads[0][1], att2.grad)


# ---------------------------------------------------------------- 5 real sampler output
def test_on_sampler_blocks_with_self_loops(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from test_graph_oracle import make_csr
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    from wholegraph_amd.torch.graph_ops import add_csr_self_loop
    n_nodes, H, F = 20011, 4, 16
    row_ptr, col = make_csr(n_nodes, 70, 41, np.int64, heavy=[(3, 4000), (4, 0)])
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    seeds = torch.from_numpy(np.random.default_rng(3).permutation(n_nodes)[:512].astype(np.int64)).cuda()
    seeds[:2] = torch.tensor([3, 4])
    target_gids, _, csr_row_ptr, csr_col_ind = g.multilayer_sample_without_replacement(seeds, [30, 30],
                                                                                       random_seeds=[7, 8])
    rng = np.random.default_rng(9)
    for i in range(2):
        rp, ci = add_csr_self_loop(csr_row_ptr[i], csr_col_ind[i])
        n_src = target_gids[i].numel()
        assert rp.dtype == torch.int32 and ci.dtype == torch.int32
        h_np, att_np = inputs(rng, n_src, H, F)
        h = dev(h_np).requires_grad_(True)
        att = dev(att_np).requires_grad_(True)
        out, alpha = mha_gat_n2n(h, att, rp, ci, H, 0.2, i == 0, return_alpha=True)
        rp_np, ci_np, al = rp.cpu().numpy(), ci.cpu().numpy(), alpha.detach().cpu().numpy()
        assert np.array_equal(bits(out), ref_out(rp_np, ci_np, h_np, al, H, i == 0).view(np.uint32))
        G_np = rng.standard_normal(tuple(out.shape)).astype(F32)
        out.backward(dev(G_np))
        gh, ga = ref_backward(rp_np, ci_np, h_np, att_np, al, G_np, H, 0.2, i == 0, chunk_edges(), node_chunk())
        assert np.array_equal(bits(h.grad), gh.view(np.uint32))
        assert np.array_equal(bits(att.grad), ga.view(np.uint32))
        h2 = dev(h_np).requires_grad_(True)
        att2 = dev(att_np).requires_grad_(True)
        want = composite(h2, att2, rp, ci, H, 0.2, i == 0)
        assert_close_scaled(out.detach(), want.detach(), 1e-5)
        want.backward(dev(G_np))
        assert_close_scaled(h.grad, h2.grad)
        assert_close_scaled(att.grad, att2.grad)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


# ---------------------------------------------------------------- 6 CuGraphGATConv
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_gat_conv_matches_composite(gpu_env, concat, bias):
    import torch
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout, H = 150, 700, 48, 24, 4
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    layer = CuGraphGATConv(cin, cout, heads=H, concat=concat, bias=bias).cuda()
    if bias:
        with torch.no_grad():
            layer.bias.normal_()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, 20)
    assert out.shape == ((n_dst, H * cout) if concat else (n_dst, cout))
    x2 = x.detach().clone().requires_grad_(True)
    ref = composite(layer.lin(x2), layer.att, rp, ci, H, layer.negative_slope, concat)
    if bias:
        ref = ref + layer.bias
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
    names = ["lin.weight", "att"] + (["bias"] if bias else [])
    assert sorted(n for n, _ in layer.named_parameters()) == sorted(names)
    got = torch.autograd.grad(out.square().sum(), [x] + [dict(layer.named_parameters())[n] for n in names])
    want = torch.autograd.grad(ref.square().sum(), [x2] + [dict(layer.named_parameters())[n] for n in names])
    for name, g, w in zip(["x"] + names, got, want):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, name
        assert_close_scaled(g, w)


# ---------------------------------------------------------------- 7 end to end
def test_two_layer_gat_trains_end_to_end(gpu_env):
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import CuGraphGATConv
    from wholegraph_amd.torch.embedding import WholeMemoryEmbeddingModule
    from wholegraph_amd.torch.graph_ops import add_csr_self_loop
    torch.manual_seed(1)
    rng = np.random.default_rng(2)
    n, k, dim, hidden, heads = 4000, 4, 32, 64, 4
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

    class TwoLayerGAT(torch.nn.Module):
        """the reference's HomoGNNModel flow for gat: sample, gather, self loops, concat hidden layer, mean last layer"""

        def __init__(self):
            super().__init__()
            self.gather_fn = WholeMemoryEmbeddingModule(emb)
            self.layers = torch.nn.ModuleList([CuGraphGATConv(dim, hidden // heads, heads=heads, concat=True),
                                               CuGraphGATConv(hidden, k, heads=heads, concat=False)])

        def forward(self, ids):
            fan = [10, 10]
            tg, _, rps, cis = g.multilayer_sample_without_replacement(ids.to(g.csr_col_ind.dtype), fan)
            x = self.gather_fn(tg[0], force_dtype=torch.float32)
            for i, layer in enumerate(self.layers):
                rp, ci = add_csr_self_loop(rps[i], cis[i])
                x = layer(x, rp, ci, fan[1 - i] + 1)
                if i == 0:
                    x = Fn.dropout(Fn.relu(x), 0.1, training=self.training)
            return x

    model = TwoLayerGAT().cuda()
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
