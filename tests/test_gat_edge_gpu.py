"""GAT attention aggregation with edge features in the logit on the MI355X
(wholegraph_amd/torch/edge_gat_aggregation.py -> csrc/kernels/gat_edge.hip).

The order of include/wholememory/wholegraph_amd_ext.h, section 2f, restated in numpy on top of test_gat_gpu's helpers
(extended here for the edge term) and compared bit for bit; alpha against a float64 softmax; the reduction to mha_gat_n2n
when the edge features are zero; torch autograd through the composite with the edge term; determinism; EdgeGATConv; and a
two-layer EdgeGATConv model trained on sampled edge attributes end to end."""
import numpy as np
import pytest

import _long_runs as LR
from test_gat_gpu import F32, U, assert_close_scaled, edge_dst, inputs, ref_alpha64, ref_out, ref_scores, seg_sum
from test_sage_agg_gpu import _planted_partition, _wm_array, bits, block, dev

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the order, restated (the edge term on top of 2c)
def ref_edge_scores(ef, att3, H):
    """s_edge [E, H]: att[2, k, :] . edge_feat[e, k, :], left to right over f"""
    E, hf = ef.shape
    F = hf // H
    ev, a2 = ef.reshape(E, H, F), att3.reshape(3, H, F)[2]
    s = np.full((E, H), -0.0, F32)
    for f in range(F):
        s = s + a2[:, f] * ev[:, :, f]
    return s


def ref_z(row_ptr, col, h, att3, s_edge, H):
    """z = (s_src[col[e]] + s_dst[d]) + s_edge[e], in that association"""
    hf = h.shape[1]
    s_src, s_dst = ref_scores(h, att3[:2 * hf], H, len(row_ptr) - 1)
    return (s_src[np.asarray(col, np.int64)] + s_dst[edge_dst(row_ptr)]) + s_edge


def ref_alpha64_edge(row_ptr, z, slope):
    """test_gat_gpu.ref_alpha64 (its bound unchanged) from the logits z that carry the edge term"""
    H = z.shape[1]
    dst = edge_dst(row_ptr)
    l = np.where(z > 0, z, F32(slope) * z).astype(np.float64)
    m = np.full((len(row_ptr) - 1, H), -np.inf)
    np.maximum.at(m, dst, l)
    w = np.exp(l - m[dst])
    den = np.zeros_like(m)
    np.add.at(den, dst, w)
    ref = w / den[dst]
    deg = np.diff(np.asarray(row_ptr, np.int64))[dst][:, None]
    spread = np.zeros_like(m)
    np.maximum.at(spread, dst, np.abs(l - m[dst]))
    bound = (8.0 + deg + spread[dst]) * 2 * U * ref + 1e-38
    return ref, bound


def test_alpha_bound_is_the_plain_ops_bound():
    """ref_alpha64_edge with a zero edge term is test_gat_gpu.ref_alpha64, value and bound"""
    rng = np.random.default_rng(1)
    row_ptr, col = block(rng, 40, 90, 12)
    h, att = inputs(rng, 90, 2, 5)
    att3 = np.concatenate([att, np.zeros(10, F32)])
    z = ref_z(row_ptr, col, h, att3, np.zeros((len(col), 2), F32), 2)
    ref, bound = ref_alpha64_edge(row_ptr, z, 0.2)
    ref0, bound0 = ref_alpha64(row_ptr, col, h, att, 2, 0.2)
    assert np.array_equal(ref, ref0) and np.array_equal(bound, bound0)


def ref_backward_edge(row_ptr, col, h, att3, ef, alpha, G, H, slope, concat, chunk, node_chunk):
    """(grad_h, grad_att [3*H*F], grad_edge_feat, dz) in the order of section 2f, from the op's alpha: test_gat_gpu.ref_backward
    with the edge term in z, plus grad_edge_feat = dz * att[2] and grad_att[2] in edge chunks of node_chunk"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, n_src, hf = len(row_ptr) - 1, h.shape[0], h.shape[1]
    F = hf // H
    E = len(col)
    hv, a, ev = h.reshape(n_src, H, F), att3.reshape(3, H, F), ef.reshape(E, H, F)
    Gk = G.reshape(n_dst, H, F) if concat else G[:, None, :] * (F32(1.0) / F32(H))
    dst = edge_dst(row_ptr)
    da = np.full((E, H), -0.0, F32)
    for f in range(F):
        da = da + Gk[dst, :, f] * hv[col, :, f]
    c = seg_sum(row_ptr, alpha * da)
    z = ref_z(row_ptr, col, h, att3, ref_edge_scores(ef, att3, H), H)
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
    ga = np.zeros((3, H, F), F32)
    for half, ds, rows_v, rows in ((0, ds_src, hv, n_src), (1, ds_dst, hv, n_dst), (2, dz, ev, E)):
        if rows == 0:
            continue
        tot = np.full((H, F), -0.0, F32)
        for q0 in range(0, rows, node_chunk):
            part = np.full((H, F), -0.0, F32)
            for j in range(q0, min(rows, q0 + node_chunk)):
                part = part + ds[j][:, None] * rows_v[j]
            tot = tot + part
        ga[half] = tot
    gef = dz[:, :, None] * a[2]
    return gh.reshape(n_src, hf), ga.reshape(-1), gef.reshape(E, hf), dz


def composite_edge(h, att3, ef, row_ptr, col, H, slope, concat):
    """test_gat_gpu.composite with att[2] . edge_feat added to the logit"""
    import torch
    n_dst = row_ptr.numel() - 1
    F = h.shape[1] // H
    hv, a = h.view(-1, H, F), att3.view(3, H, F)
    s_src = (hv * a[0]).sum(-1)
    s_dst = (hv[:n_dst] * a[1]).sum(-1)
    s_edge = (ef.view(-1, H, F) * a[2]).sum(-1)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=h.device), deg)
    col = col.long()
    l = torch.nn.functional.leaky_relu(s_src[col] + s_dst[dst] + s_edge, slope)
    m = torch.full((n_dst, H), -float("inf"), device=h.device, dtype=h.dtype).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=h.device, dtype=h.dtype).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=h.device, dtype=h.dtype).index_add_(0, dst, alpha[:, :, None] * hv[col])
    return o.reshape(n_dst, H * F) if concat else o.mean(1)


# ---------------------------------------------------------------- blocks and inputs
N_SRC = 200


def edge_block(rng, C, n_edges=None, n_dst=60):
    """targets of degree 0, 1, 9 (more than one batch of 8, not a multiple) and 70 (more than 64 lanes) among random ones;
    source 5 with C + 37 edges (a chunked run with a ragged last chunk), source 9 with none; optionally exactly n_edges
    edges"""
    deg = rng.integers(0, 41, n_dst)
    deg[:4] = (0, 1, 9, 70)
    deg[::7][1:] = 0
    if n_edges is not None:
        deg[-1] = 0
        assert n_edges - deg.sum() > 0
        deg[-1] = n_edges - deg.sum()
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    E = int(row_ptr[-1])
    col = rng.integers(0, N_SRC, E).astype(np.int32)
    col[col == 5] = 6
    col[col == 9] = 10
    col[rng.choice(E, C + 37, replace=False)] = 5
    counts = np.bincount(col, minlength=N_SRC)
    assert counts[5] == C + 37 and (C + 37) % C and counts[9] == 0
    return row_ptr, col


def edge_inputs(rng, E, H, F, scale=0.5):
    h, att = inputs(rng, N_SRC, H, F, scale)
    a2 = (scale * rng.standard_normal(H * F) / np.sqrt(F)).astype(F32)
    return h, np.concatenate([att, a2]), rng.standard_normal((E, H * F)).astype(F32)


def run_op(h_np, att_np, ef, row_ptr, col, H, concat, G_np):
    """(out, alpha, edge_scores, grad_h, grad_att, grad_edge_feat) of the op; `ef` a device tensor (leaf)"""
    from wholegraph_amd.torch.edge_gat_aggregation import CscGatEdgeConv
    h = dev(h_np).requires_grad_(True)
    att = dev(att_np).requires_grad_(True)
    ef.requires_grad_(True)
    out, alpha, es = CscGatEdgeConv.apply(h, att, ef, dev(row_ptr), dev(col), H, 0.2, concat)
    out.backward(dev(G_np))
    return out.detach(), alpha, es, h.grad, att.grad, ef.grad


def check_bits(h_np, att_np, ef_np, ef, row_ptr, col, H, concat, rng):
    """test 1 and test 2 on one block"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    n_dst, hf = len(row_ptr) - 1, h_np.shape[1]
    G_np = rng.standard_normal((n_dst, hf if concat else hf // H)).astype(F32)
    out, alpha, es, gh, ga, gef = run_op(h_np, att_np, ef, row_ptr, col, H, concat, G_np)
    assert out.shape == G_np.shape and alpha.shape == (len(col), H) and es.shape == (len(col), H)
    assert gef.shape == ef_np.shape and ga.shape == (3 * hf,)
    s_edge = ref_edge_scores(ef_np, att_np, H)
    assert np.array_equal(bits(es), s_edge.view(np.uint32)), "edge_scores"
    al = alpha.cpu().numpy()
    ref, bound = ref_alpha64_edge(row_ptr, ref_z(row_ptr, col, h_np, att_np, s_edge, H), 0.2)
    assert (np.abs(al - ref) <= bound).all(), "alpha off by %g" % float(np.max(np.abs(al - ref) / (ref + 1e-30)))
    assert np.array_equal(bits(out), ref_out(row_ptr, col, h_np, al, H, concat).view(np.uint32)), "out"
    rgh, rga, rgef, _ = ref_backward_edge(row_ptr, col, h_np, att_np, ef_np, al, G_np, H, 0.2, concat, chunk_edges(),
                                          node_chunk())
    assert np.array_equal(bits(gh), rgh.view(np.uint32)), "grad_h"
    for half in range(3):
        assert np.array_equal(bits(ga)[half * hf:(half + 1) * hf], rga.view(np.uint32)[half * hf:(half + 1) * hf]), \
            "grad_att[%d]" % half
    assert np.array_equal(bits(gef), rgef.view(np.uint32)), "grad_edge_feat"


# ---------------------------------------------------------------- 1, 2 bits against the stated order, alpha
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H", [1, 3, 4])
@pytest.mark.parametrize("F", [1, 3, 4, 8, 33])
def test_bits_against_stated_order(gpu_env, F, H, concat):
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(1000 + 100 * F + 10 * H + concat)
    row_ptr, col = edge_block(rng, chunk_edges())
    h, att, ef = edge_inputs(rng, len(col), H, F)
    check_bits(h, att, ef, dev(ef), row_ptr, col, H, concat, rng)


def test_bits_ragged_last_edge_chunk(gpu_env):
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    rng = np.random.default_rng(77)
    E = 2 * node_chunk() + 17
    row_ptr, col = edge_block(rng, chunk_edges(), n_edges=E)
    assert len(col) == E
    h, att, ef = edge_inputs(rng, E, 4, 8)
    check_bits(h, att, ef, dev(ef), row_ptr, col, 4, True, rng)


@pytest.mark.parametrize("F", [5, 8])
def test_bits_with_runs_of_more_than_one_batch_of_partials(gpu_env, F):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    C, H = chunk_edges(), 2
    rng = np.random.default_rng(900 + F)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    h, att = inputs(rng, LR.N_SRC, H, F)
    att = np.concatenate([att, (0.5 * rng.standard_normal(H * F) / np.sqrt(F)).astype(F32)])
    ef = rng.standard_normal((len(col), H * F)).astype(F32)
    for concat in (True, False):
        check_bits(h, att, ef, dev(ef), row_ptr, col, H, concat, rng)


def test_bits_strided_unaligned_edge_feat(gpu_env):
    """edge_feat as a column slice of a wider tensor (stride H*F + 9, start 12 bytes off): the element-wise instantiation
    at F = 8"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(78)
    H, F = 4, 8
    row_ptr, col = edge_block(rng, chunk_edges())
    h, att, _ = edge_inputs(rng, len(col), H, F)
    wide = rng.standard_normal((len(col), H * F + 9)).astype(F32)
    view = dev(wide)[:, 3:3 + H * F]
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0 and view.stride(0) == H * F + 9
    check_bits(h, att, wide[:, 3:3 + H * F].copy(), view, row_ptr, col, H, True, rng)


@pytest.mark.parametrize("n_dst", [0, 6])
def test_bits_empty_blocks(gpu_env, n_dst):
    """n_dst = 0, then E = 0 with targets"""
    rng = np.random.default_rng(79)
    H, F = 2, 8
    h, att, ef = edge_inputs(rng, 0, H, F)
    row_ptr, col = np.zeros(n_dst + 1, np.int32), np.zeros(0, np.int32)
    check_bits(h, att, ef, dev(ef), row_ptr, col, H, True, rng)
    G_np = np.ones((n_dst, H * F), F32)
    out, _, _, gh, ga, _ = run_op(h, att, dev(ef), row_ptr, col, H, True, G_np)
    assert not out.any() and not gh.any() and not ga.any()


# ---------------------------------------------------------------- 3 reduction to the plain op
@pytest.mark.parametrize("H,F,concat", [(4, 8, True), (3, 33, False), (1, 3, True), (4, 32, False)])
def test_zero_edge_features_reduce_to_mha_gat_n2n(gpu_env, H, F, concat):
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.edge_gat_aggregation import mha_gat_n2n_edge
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    rng = np.random.default_rng(400 + 10 * H + F)
    hf = H * F
    row_ptr, col = edge_block(rng, chunk_edges())
    h_np, att_np, _ = edge_inputs(rng, len(col), H, F)
    ef_np = np.zeros((len(col), hf), F32)
    z = ref_z(row_ptr, col, h_np, att_np, ref_edge_scores(ef_np, att_np, H), H)
    assert (z != 0).all(), "z = +-0 would let the sign of the zero edge score show"
    G = dev(rng.standard_normal((len(row_ptr) - 1, hf if concat else F)).astype(F32))
    rp, ci = dev(row_ptr), dev(col)
    h = dev(h_np).requires_grad_(True)
    att = dev(att_np).requires_grad_(True)
    ef = dev(ef_np).requires_grad_(True)
    out, alpha = mha_gat_n2n_edge(h, att, ef, rp, ci, H, 0.2, concat, return_alpha=True)
    out.backward(G)
    h0 = dev(h_np).requires_grad_(True)
    att0 = dev(att_np[:2 * hf]).requires_grad_(True)
    out0, alpha0 = mha_gat_n2n(h0, att0, rp, ci, H, 0.2, concat, return_alpha=True)
    out0.backward(G)
    assert np.array_equal(bits(out), bits(out0)) and np.array_equal(bits(alpha), bits(alpha0))
    assert np.array_equal(bits(h.grad), bits(h0.grad))
    assert np.array_equal(bits(att.grad)[:2 * hf], bits(att0.grad))
    assert not att.grad[2 * hf:].any(), "grad_att[2] is +-0 over zero edge features"
    _, _, rgef, dz = ref_backward_edge(row_ptr, col, h_np, att_np, ef_np, alpha.cpu().numpy(), G.cpu().numpy(), H, 0.2,
                                       concat, chunk_edges(), node_chunk())
    assert dz.any() and np.array_equal(bits(ef.grad), rgef.view(np.uint32)), "grad_edge_feat = dz * att[2]"


# ---------------------------------------------------------------- 4 against autograd
@pytest.mark.parametrize("H,F,concat", [(4, 8, True), (3, 33, False), (1, 1, True), (4, 32, False)])
def test_against_autograd_composite(gpu_env, H, F, concat):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.edge_gat_aggregation import mha_gat_n2n_edge
    rng = np.random.default_rng(500 + 10 * H + F)
    row_ptr, col = edge_block(rng, chunk_edges())
    h_np, att_np, ef_np = edge_inputs(rng, len(col), H, F)
    G = dev(rng.standard_normal((len(row_ptr) - 1, H * F if concat else F)).astype(F32))
    rp, ci = dev(row_ptr), dev(col)
    leaves = [dev(a).requires_grad_(True) for a in (h_np, att_np, ef_np)]
    out = mha_gat_n2n_edge(leaves[0], leaves[1], leaves[2], rp, ci, H, 0.2, concat)
    out.backward(G)
    leaves64 = [dev(a.astype(np.float64)).requires_grad_(True) for a in (h_np, att_np, ef_np)]
    want = composite_edge(leaves64[0], leaves64[1], leaves64[2], rp, ci, H, 0.2, concat)
    want.backward(G.double())
    assert_close_scaled(out.detach(), want.detach(), 1e-5)
    for name, got, ref in zip(("h", "att", "edge_feat"), leaves, leaves64):
        assert torch.isfinite(got.grad).all(), name
        assert_close_scaled(got.grad, ref.grad)


# ---------------------------------------------------------------- 5 determinism
def test_two_calls_give_equal_bits(gpu_env):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(6)
    H, F = 4, 32
    row_ptr, col = edge_block(rng, chunk_edges(), n_edges=5000, n_dst=150)
    h_np, att_np, ef_np = edge_inputs(rng, len(col), H, F)
    G_np = rng.standard_normal((len(row_ptr) - 1, H * F)).astype(F32)
    a = run_op(h_np, att_np, dev(ef_np), row_ptr, col, H, True, G_np)
    b = run_op(h_np, att_np, dev(ef_np), row_ptr, col, H, True, G_np)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------- 6 EdgeGATConv
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_edge_gat_conv_matches_composite(gpu_env, concat, bias):
    import torch
    from wholegraph_amd.torch.cugraphops import EdgeGATConv
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout, H, edim = 150, 700, 48, 24, 4, 5
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    layer = EdgeGATConv(cin, cout, edim, heads=H, concat=concat, bias=bias).cuda()
    if bias:
        with torch.no_grad():
            layer.bias.normal_()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    ea = dev(rng.standard_normal((len(col), edim)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, ea, 20)
    assert out.shape == ((n_dst, H * cout) if concat else (n_dst, cout))
    x2 = x.detach().clone().requires_grad_(True)
    ea2 = ea.detach().clone().requires_grad_(True)
    ref = composite_edge(layer.lin(x2), layer.att, layer.lin_edge(ea2), rp, ci, H, layer.negative_slope, concat)
    if bias:
        ref = ref + layer.bias
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
    names = ["lin.weight", "lin_edge.weight", "att"] + (["bias"] if bias else [])
    assert sorted(n for n, _ in layer.named_parameters()) == sorted(names)
    params = [dict(layer.named_parameters())[n] for n in names]
    got = torch.autograd.grad(out.square().sum(), [x, ea] + params)
    want = torch.autograd.grad(ref.square().sum(), [x2, ea2] + params)
    for name, g, w in zip(["x", "edge_attr"] + names, got, want):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, name
        assert_close_scaled(g, w)


def test_edge_gat_conv_scalar_attribute_autocast_and_dtypes(gpu_env):
    import torch
    from wholegraph_amd.torch.cugraphops import EdgeGATConv
    from wholegraph_amd.torch.edge_gat_aggregation import mha_gat_n2n_edge
    torch.manual_seed(3)
    rng = np.random.default_rng(22)
    n_dst, n_src, H, F = 90, 300, 2, 8
    row_ptr, col = block(rng, n_dst, n_src, 12)
    rp, ci = dev(row_ptr), dev(col)
    layer = EdgeGATConv(16, F, 1, heads=H).cuda()
    x = dev(rng.standard_normal((n_src, 16)).astype(F32))
    w = dev(rng.random(len(col)).astype(F32))
    assert torch.equal(layer(x, rp, ci, w).view(torch.int32), layer(x, rp, ci, w[:, None]).view(torch.int32))
    # autocast: 16-bit h / edge_feat are widened on the way in, the op runs in fp32
    h16 = dev(rng.standard_normal((n_src, H * F)).astype(F32)).bfloat16()
    ef16 = dev(rng.standard_normal((len(col), H * F)).astype(F32)).bfloat16()
    att = dev(rng.standard_normal(3 * H * F).astype(F32))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = mha_gat_n2n_edge(h16, att, ef16, rp, ci, H)
    assert got.dtype == torch.float32
    assert torch.equal(got, mha_gat_n2n_edge(h16.float(), att, ef16.float(), rp, ci, H))
    with pytest.raises(TypeError, match="float32"):
        mha_gat_n2n_edge(h16, att, ef16.float(), rp, ci, H)
    with pytest.raises(TypeError, match="float32"):
        mha_gat_n2n_edge(h16.float(), att, ef16.half(), rp, ci, H)


# ---------------------------------------------------------------- 7 end to end
def test_two_layer_edge_gat_trains_on_sampled_edge_attributes(gpu_env):
    """step count and criterion of test_gat_gpu.test_two_layer_gat_trains_end_to_end; the blocks as sampled (no self loops)"""
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import EdgeGATConv
    torch.manual_seed(1)
    rng = np.random.default_rng(2)
    n, k, dim, hidden, heads = 2000, 4, 32, 64, 4
    row_ptr, col, labels_np = _planted_partition(n, k, rng)
    centres = rng.standard_normal((k, dim)).astype(F32)
    feats = torch.from_numpy((0.5 * centres[labels_np] + rng.standard_normal((n, dim)).astype(F32)).astype(F32)).cuda()
    src_of_edge = np.repeat(np.arange(n), np.diff(row_ptr))
    attr = ((labels_np[src_of_edge] == labels_np[col]) + 0.1 * rng.standard_normal(len(col))).astype(F32)
    wrow, wcol, wattr = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col), _wm_array(gpu_env, attr)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    g.set_edge_attribute("same", wattr)

    class TwoLayerEdgeGAT(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = torch.nn.ModuleList([EdgeGATConv(dim, hidden // heads, 1, heads=heads, concat=True),
                                               EdgeGATConv(hidden, k, 1, heads=heads, concat=False)])

        def forward(self, ids):
            tg, _, rps, cis, attrs = g.multilayer_sample_with_edge_attributes(ids.to(g.csr_col_ind.dtype), [10, 10],
                                                                              ["same"])
            x = feats[tg[0]]
            for i, layer in enumerate(self.layers):
                assert attrs[i]["same"].shape == cis[i].shape
                x = layer(x, rps[i], cis[i], attrs[i]["same"])
                if i == 0:
                    x = Fn.dropout(Fn.relu(x), 0.1, training=self.training)
            return x

    model = TwoLayerEdgeGAT().cuda()
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
        if step == 0:
            for name, p in model.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all(), name
            assert all(layer.lin_edge.weight.grad.abs().sum() > 0 for layer in model.layers)
        opt.step()
        if step == 0:
            for name, p in model.named_parameters():
                assert torch.isfinite(p).all(), name
        losses.append(float(loss.detach()))
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    assert np.isfinite(losses).all()
    assert last < 0.6 * first, "loss %.3f -> %.3f" % (first, last)
    wgth.destroy_wholememory_tensor(wattr)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
