"""GATv2 attention aggregation on the MI355X (wholegraph_amd/torch/gatv2_aggregation.py -> csrc/kernels/gatv2.hip).

The logits are restated bit for bit (tree included) and alpha is checked against a float64 softmax of them; out and the
three gradients are checked bit for bit against a numpy restatement of the order the header states
(include/wholememory/wholegraph_amd_ext.h, section 2g), fed the op's own alpha, and with allclose against torch autograd
through an index_select / scatter-max / index_add_ composite. Then GATv2Conv against the composite, and a two-layer
"gatv2" HomoGNNModel trained end to end on a planted-partition graph held in WholeMemory."""
import random
import types

import numpy as np
import pytest

import _long_runs as LR
from test_gat_gpu import U, assert_close_scaled, edge_dst, ref_out, seg_sum
from test_sage_agg_gpu import _planted_partition, _wm_array, bits, block, dev

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (2, 3), (3, 4), (4, 8), (4, 32), (2, 128), (8, 64)]


# ---------------------------------------------------------------- the order, restated
def tree_sum(q):
    """the balanced tree of adjacent pairs over the last axis, padded with +0.0 to a power of two"""
    F = q.shape[-1]
    Fp = 1
    while Fp < F:
        Fp *= 2
    if Fp > F:
        q = np.concatenate([q, np.zeros(q.shape[:-1] + (Fp - F,), F32)], axis=-1)
    while q.shape[-1] > 1:
        q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0]


def ref_u(row_ptr, col, hs, hd, H):
    F = hs.shape[1] // H
    dst = edge_dst(row_ptr)
    return hs[np.asarray(col, np.int64)].reshape(-1, H, F) + hd[dst].reshape(-1, H, F)


def ref_logits(row_ptr, col, hs, hd, att, H, slope):
    u = ref_u(row_ptr, col, hs, hd, H)
    v = np.where(u > 0, u, F32(slope) * u).astype(F32)
    return tree_sum(att.reshape(H, -1) * v), u, v


def ref_alpha64(row_ptr, l32):
    """float64 softmax over each target's edges of the fp32 logits, and the bound test_gat_gpu.ref_alpha64 takes: a few
    fp32 ulp plus the rounding of den (deg terms) and of l - max"""
    dst = edge_dst(row_ptr)
    l = l32.astype(np.float64)
    m = np.full((len(row_ptr) - 1, l.shape[1]), -np.inf)
    np.maximum.at(m, dst, l)
    w = np.exp(l - m[dst])
    den = np.zeros_like(m)
    np.add.at(den, dst, w)
    ref = w / den[dst]
    deg = np.diff(np.asarray(row_ptr, np.int64))[dst][:, None]
    spread = np.zeros_like(m)
    np.maximum.at(spread, dst, np.abs(l - m[dst]))
    return ref, (8.0 + deg + spread[dst]) * 2 * U * ref + 1e-38


def ref_backward(row_ptr, col, hs, hd, att, alpha, G, H, slope, concat, chunk, node_chunk):
    """(grad_h_src, grad_h_dst, grad_att) in the stated order, from the op's alpha"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, n_src, hf = len(row_ptr) - 1, hs.shape[0], hs.shape[1]
    F = hf // H
    a = att.reshape(H, F)
    Gk = G.reshape(n_dst, H, F) if concat else G[:, None, :] * (F32(1.0) / F32(H))
    dst = edge_dst(row_ptr)
    _, u, v = ref_logits(row_ptr, col, hs, hd, att, H, slope)
    da = tree_sum(Gk[dst] * hs[col].reshape(-1, H, F))
    c = seg_sum(row_ptr, alpha * da)
    dl = (alpha * (da - c[dst])).astype(F32)
    g = np.where(u > 0, a, a * F32(slope)).astype(F32)
    du = dl[:, :, None] * g
    ghd = seg_sum(row_ptr, du)
    terms = (alpha[:, :, None] * Gk[dst]) + du
    ghs = np.zeros((n_src, H, F), F32)
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(n_src + 1))
    for j in np.nonzero(np.diff(starts))[0]:
        edges = order[starts[j]:starts[j + 1]]
        p = None
        for c0 in range(0, len(edges), chunk):
            pp = terms[edges[c0]].copy()
            for e in edges[c0 + 1:c0 + chunk]:
                pp = pp + terms[e]
            p = pp if p is None else p + pp
        ghs[j] = p
    A = seg_sum(row_ptr, dl[:, :, None] * v)
    ga = np.zeros((H, F), F32)
    if n_dst:
        tot = np.full((H, F), -0.0, F32)
        for q0 in range(0, n_dst, node_chunk):
            part = np.full((H, F), -0.0, F32)
            for d in range(q0, min(n_dst, q0 + node_chunk)):
                part = part + A[d]
            tot = tot + part
        ga = tot
    return ghs.reshape(n_src, hf), ghd.reshape(n_dst, hf), ga.reshape(-1)


def composite(hs, hd, att, row_ptr, col, H, slope, concat):
    """torch autograd reference: index_select, a scatter-max / exp / index_add_ softmax, index_add_"""
    import torch
    n_dst = row_ptr.numel() - 1
    F = hs.shape[1] // H
    hv, dv, a = hs.view(-1, H, F), hd.view(-1, H, F), att.view(H, F)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=hs.device), deg)
    col = col.long()
    l = (torch.nn.functional.leaky_relu(hv[col] + dv[dst], slope) * a).sum(-1)
    m = torch.full((n_dst, H), -float("inf"), device=hs.device, dtype=hs.dtype).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=hs.device, dtype=hs.dtype).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=hs.device, dtype=hs.dtype).index_add_(0, dst, alpha[:, :, None] * hv[col])
    return o.reshape(n_dst, H * F) if concat else o.mean(1)


def inputs(rng, n_src, n_dst, H, F, scale=0.5):
    hs = rng.standard_normal((n_src, H * F)).astype(F32)
    hd = rng.standard_normal((n_dst, H * F)).astype(F32)
    att = (scale * rng.standard_normal(H * F) / np.sqrt(F)).astype(F32)
    return hs, hd, att


_BLOCK = {}


def hub_block(C):
    """targets of degree 0, 1, 8, 9 and 17 (around the batch of 8 rows), duplicate edges, source 0 with 2C + 3 edges
    (chunks, the last one partial) and source 1 with exactly C; built once and shared"""
    if C not in _BLOCK:
        rng = np.random.default_rng(77)
        n_dst, n_src = 140, 300
        deg = rng.integers(0, 25, n_dst)
        deg[:5] = (0, 1, 8, 9, 17)
        deg[5:9] = (2 * C, C, C // 2, 9)
        row_ptr = np.zeros(n_dst + 1, np.int32)
        np.cumsum(deg, out=row_ptr[1:])
        E = int(row_ptr[-1])
        col = rng.integers(2, n_src, E).astype(np.int32)
        pos = rng.permutation(np.arange(int(row_ptr[5]), E))[:3 * C + 3]
        col[pos[:2 * C + 3]] = 0
        col[pos[2 * C + 3:]] = 1
        col[int(row_ptr[4]) + 1] = col[int(row_ptr[4])]   # a duplicate edge in the target of degree 17
        counts = np.bincount(col, minlength=n_src)
        assert counts[0] == 2 * C + 3 and counts[1] == C and (counts == 0).any()
        _BLOCK[C] = (row_ptr, col, n_dst, n_src)
    return _BLOCK[C]


def run_op(hs_t, hd_t, att_np, row_ptr, col, G_np, H, slope, concat, need=(True, True, True)):
    """(out, alpha, grads) of one forward + backward; grads[i] is None where need[i] is False"""
    from wholegraph_amd.torch.gatv2_aggregation import mha_gat_v2_n2n
    hs = hs_t.detach().requires_grad_(need[0])
    hd = hd_t.detach().requires_grad_(need[1])
    att = dev(att_np).requires_grad_(need[2])
    out, alpha = mha_gat_v2_n2n(hs, hd, att, dev(row_ptr), dev(col), H, slope, concat, return_alpha=True)
    out.backward(dev(G_np))
    return out.detach(), alpha.detach(), [t.grad for t in (hs, hd, att)]


def check_all(hs_np, hd_np, att_np, row_ptr, col, H, slope, concat, rng, hs_t=None, hd_t=None, loose=True):
    """every output of the op against the restatement (alpha within its bound, the rest bit for bit) and, with `loose`,
    against torch autograd through the composite; returns the op's outputs"""
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    n_dst, hf = len(row_ptr) - 1, hs_np.shape[1]
    G_np = rng.standard_normal((n_dst, hf if concat else hf // H)).astype(F32)
    hs_t = dev(hs_np) if hs_t is None else hs_t
    hd_t = dev(hd_np) if hd_t is None else hd_t
    out, alpha, grads = run_op(hs_t, hd_t, att_np, row_ptr, col, G_np, H, slope, concat)
    assert out.shape == ((n_dst, hf) if concat else (n_dst, hf // H)) and alpha.shape == (len(col), H)
    al = alpha.cpu().numpy()
    l32, _, _ = ref_logits(row_ptr, col, hs_np, hd_np[:n_dst], att_np, H, slope)
    ref, bound = ref_alpha64(row_ptr, l32)
    print("alpha: max |err| / bound = %.3g" % (float(np.max(np.abs(al - ref) / bound)) if len(col) else 0.0))
    assert (np.abs(al - ref) <= bound).all(), "alpha off by %g" % float(np.max(np.abs(al - ref) / (ref + 1e-30)))
    assert np.array_equal(bits(out), ref_out(row_ptr, col, hs_np, al, H, concat).view(np.uint32))
    ghs, ghd, ga = ref_backward(row_ptr, col, hs_np, hd_np[:n_dst], att_np, al, G_np, H, slope, concat, chunk_edges(),
                                node_chunk())
    assert np.array_equal(bits(grads[0]), ghs.view(np.uint32)), "grad_h_src"
    assert np.array_equal(bits(grads[1])[:n_dst], ghd.view(np.uint32)), "grad_h_dst"
    assert not grads[1][n_dst:].any()
    assert np.array_equal(bits(grads[2]), ga.view(np.uint32)), "grad_att"
    if loose:   # the tolerances test_gat_gpu.py takes for the same comparison
        hs2 = dev(hs_np).requires_grad_(True)
        hd2 = dev(hd_np).requires_grad_(True)
        att2 = dev(att_np).requires_grad_(True)
        want = composite(hs2, hd2, att2, dev(row_ptr), dev(col), H, slope, concat)
        assert_close_scaled(out, want.detach(), 1e-5)
        want.backward(dev(G_np))
        for got, w in zip(grads, (hs2.grad, hd2.grad, att2.grad)):
            assert_close_scaled(got, w)
    return out, alpha, grads, G_np


# ---------------------------------------------------------------- 1 every lane mapping, forward and backward
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("concat", [True, False])
def test_bitwise_on_hub_block(gpu_env, H, F, concat):
    """Fp = 1, tree padding (F = 3), one lane per head (F = 4), heads sharing a wave, lane groups of 16 / 32 / 64, rows with
    more pieces than lanes (8 x 64); negative_slope 0.2 with concat, 0.0 with the head mean"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(1000 + 10 * H + F + concat)
    hs, hd, att = inputs(rng, n_src, n_dst, H, F)
    check_all(hs, hd, att, row_ptr, col, H, 0.2 if concat else 0.0, concat, rng)


@pytest.mark.parametrize("F", [5, 8])
def test_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, F):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    C, H = chunk_edges(), 2
    rng = np.random.default_rng(900 + F)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    hs, hd, att = inputs(rng, LR.N_SRC, LR.N_DST, H, F)
    for concat in (True, False):
        check_all(hs, hd, att, row_ptr, col, H, 0.2, concat, rng, loose=False)


@pytest.mark.parametrize("concat,slope", [(True, 0.0), (False, 0.2)])
def test_bitwise_other_slope(gpu_env, concat, slope):
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(5)
    hs, hd, att = inputs(rng, n_src, n_dst, 4, 8)
    check_all(hs, hd, att, row_ptr, col, 4, slope, concat, rng)


def test_u_exactly_zero_takes_the_slope_branch(gpu_env):
    rng = np.random.default_rng(6)
    H, F, n_dst, n_src = 4, 8, 40, 90
    row_ptr, col = block(rng, n_dst, n_src, 12)
    hs, hd, att = inputs(rng, n_src, n_dst, H, F)
    for d in range(1, n_dst, 3):   # the first edge of every third target: u = 0.0 in every column
        if row_ptr[d + 1] > row_ptr[d]:
            hd[d] = -hs[col[row_ptr[d]]]
    u = ref_u(row_ptr, col, hs, hd, H)
    assert (u == 0).all(axis=(1, 2)).sum() >= 5
    check_all(hs, hd, att, row_ptr, col, H, 0.2, True, rng)


# ---------------------------------------------------------------- 2 the element-wise path gives the same bits
def test_misaligned_strided_views_equal_the_16_byte_path(gpu_env):
    import torch
    rng = np.random.default_rng(7)
    H, F, n_dst, n_src = 4, 8, 97, 260
    row_ptr, col = block(rng, n_dst, n_src, 30)
    wide_s = rng.standard_normal((n_src, H * F + 9)).astype(F32)
    wide_d = rng.standard_normal((n_dst + 3, H * F + 2)).astype(F32)
    _, _, att = inputs(rng, n_src, n_dst, H, F)
    hs_v = dev(wide_s)[:, 3:3 + H * F]   # row stride H*F + 9, offset 3 floats: not 16-byte aligned
    hd_v = dev(wide_d)[:, 1:1 + H * F]   # h_dst as a strided view, with rows behind the targets
    assert not hs_v.is_contiguous() and not hd_v.is_contiguous() and hs_v.data_ptr() % 16
    hs, hd = wide_s[:, 3:3 + H * F].copy(), wide_d[:, 1:1 + H * F].copy()
    for concat in (True, False):
        out, alpha, grads, G = check_all(hs, hd, att, row_ptr, col, H, 0.2, concat, np.random.default_rng(8), hs_t=hs_v,
                                         hd_t=hd_v, loose=False)
        out2, alpha2, grads2 = run_op(dev(hs), dev(hd), att, row_ptr, col, G, H, 0.2, concat)   # aligned: the lane-split tree
        for a, b in zip([out, alpha] + grads, [out2, alpha2] + grads2):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------- 3 node chunks of grad_att, self loops, empty blocks
def test_grad_att_over_node_chunks(gpu_env):
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    N = node_chunk()
    rng = np.random.default_rng(9)
    H, F, n_dst = 1, 4, 2 * N + 5
    n_src = n_dst + 40
    row_ptr, col = block(rng, n_dst, n_src, 3)
    hs, hd, att = inputs(rng, n_src, n_dst, H, F)
    check_all(hs, hd, att, row_ptr, col, H, 0.2, True, rng)


def test_self_loops_from_add_csr_self_loop(gpu_env):
    from wholegraph_amd.torch.graph_ops import add_csr_self_loop
    rng = np.random.default_rng(10)
    H, F, n_dst, n_src = 2, 16, 60, 200
    row_ptr, col = block(rng, n_dst, n_src, 9)
    rp, ci = add_csr_self_loop(dev(row_ptr), dev(col))
    rp_np, ci_np = rp.cpu().numpy(), ci.cpu().numpy()
    assert len(ci_np) == len(col) + n_dst and (np.diff(rp_np) >= 1).all()
    hs, hd, att = inputs(rng, n_src, n_dst, H, F)
    check_all(hs, hd, att, rp_np, ci_np, H, 0.2, False, rng)


def test_empty_blocks(gpu_env):
    rng = np.random.default_rng(11)
    H, F, n_src = 2, 8, 50
    for n_dst in (0, 6):   # n_dst = 0, then E = 0 with targets
        hs, hd, att = inputs(rng, n_src, n_dst, H, F)
        rp = np.zeros(n_dst + 1, np.int32)
        for concat in (True, False):
            out, alpha, grads, _ = check_all(hs, hd, att, rp, np.zeros(0, np.int32), H, 0.2, concat, rng, loose=False)
            assert not out.any() and all(not g.any() for g in grads)
            assert all(np.array_equal(bits(g), np.zeros(g.shape, np.uint32)) for g in [out] + grads)   # +0.0


# ---------------------------------------------------------------- 4 reproducibility, gradients on their own
def test_identical_calls_and_single_gradients_give_identical_bits(gpu_env):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(12)
    H, F = 4, 32
    hs, hd, att = inputs(rng, n_src, n_dst, H, F)
    G = rng.standard_normal((n_dst, H * F)).astype(F32)
    hs_t, hd_t = dev(hs), dev(hd)
    full = run_op(hs_t, hd_t, att, row_ptr, col, G, H, 0.2, True)
    again = run_op(hs_t, hd_t, att, row_ptr, col, G, H, 0.2, True)
    for a, b in zip(full[:2] + tuple(full[2]), again[:2] + tuple(again[2])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for i in range(3):
        need = tuple(k == i for k in range(3))
        _, _, grads = run_op(hs_t, hd_t, att, row_ptr, col, G, H, 0.2, True, need)
        assert [g is not None for g in grads] == list(need)
        assert torch.equal(grads[i].view(torch.int32), full[2][i].view(torch.int32))


# ---------------------------------------------------------------- 5 GATv2Conv
@pytest.mark.parametrize("share", [False, True])
def test_gatv2_conv_matches_composite(gpu_env, share):
    import torch
    from wholegraph_amd.torch.cugraphops import GATv2Conv
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout, H = 150, 700, 48, 24, 4
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    for concat in (True, False):
        layer = GATv2Conv(cin, cout, heads=H, concat=concat, share_weights=share).cuda()
        with torch.no_grad():
            layer.bias.normal_()
        x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
        out = layer(x, rp, ci, 20)
        assert out.shape == ((n_dst, H * cout) if concat else (n_dst, cout))
        x2 = x.detach().clone().requires_grad_(True)
        ref = composite(layer.lin_src(x2), layer.lin_dst(x2[:n_dst]), layer.att, rp, ci, H, layer.negative_slope,
                        concat) + layer.bias
        assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
        names = ["lin_src.weight", "att", "bias"] + ([] if share else ["lin_dst.weight"])
        params = dict(layer.named_parameters())
        assert sorted(params) == sorted(names)
        got = torch.autograd.grad(out.square().sum(), [x] + [params[n] for n in names])
        want = torch.autograd.grad(ref.square().sum(), [x2] + [params[n] for n in names])
        for name, g, w in zip(["x"] + names, got, want):
            assert torch.isfinite(g).all() and g.abs().sum() > 0, name
            assert_close_scaled(g, w)


def test_gatv2_conv_under_autocast_and_16_bit_rows_outside_it(gpu_env):
    import torch
    from wholegraph_amd.torch.cugraphops import GATv2Conv
    from wholegraph_amd.torch.gatv2_aggregation import mha_gat_v2_n2n
    torch.manual_seed(3)
    rng = np.random.default_rng(22)
    n_dst, n_src, cin, cout, H = 80, 300, 32, 16, 2
    row_ptr, col = block(rng, n_dst, n_src, 12)
    rp, ci = dev(row_ptr), dev(col)
    layer = GATv2Conv(cin, cout, heads=H).cuda()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h_src, h_dst = layer.lin_src(x), layer.lin_dst(x[:n_dst])
        assert h_src.dtype == torch.bfloat16
        out = layer(x, rp, ci, 12)
    assert out.dtype == torch.float32
    # the op saw the bf16 Linear outputs widened to fp32
    want = mha_gat_v2_n2n(h_src.float(), h_dst.float(), layer.att, rp, ci, H) + layer.bias
    assert torch.equal(out.detach().view(torch.int32), want.detach().view(torch.int32))
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="float32"):
            mha_gat_v2_n2n(h_src.detach().to(dt), h_dst.detach().float(), layer.att, rp, ci, H)
        with pytest.raises(TypeError, match="float32"):
            mha_gat_v2_n2n(h_src.detach().float(), h_dst.detach().to(dt), layer.att, rp, ci, H)


# ---------------------------------------------------------------- 6 end to end
def _train_gatv2(comm, seed):
    """a 2-layer, 2-head "gatv2" HomoGNNModel on the planted-partition graph of the GAT end-to-end test: the losses, the
    accuracy and the final evaluation logits"""
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    torch.manual_seed(seed)
    random.seed(seed)   # (the sampler draws its per-hop seeds from `random`)
    rng = np.random.default_rng(2)
    n, k, dim = 4000, 4, 32
    row_ptr, col, labels_np = _planted_partition(n, k, rng)
    centres = rng.standard_normal((k, dim)).astype(F32)
    feats = (0.5 * centres[labels_np] + rng.standard_normal((n, dim)).astype(F32)).astype(F32)
    wrow, wcol = _wm_array(comm, row_ptr), _wm_array(comm, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [n, dim])
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(torch.from_numpy(feats).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "adam", {})
    torch.cuda.synchronize()
    before = emb.get_embedding_tensor().get_local_tensor()[0].clone()
    wgth.set_framework("cugraph")
    args = types.SimpleNamespace(model="gatv2", hiddensize=64, layernum=2, classnum=k, dropout=0.1, neighbors="10,10",
                                 inferencesample="10,10", heads=2)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    assert [type(l).__name__ for l in model.gnn_layers] == ["GATv2Conv", "GATv2Conv"] and model.add_self_loop
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
    after = emb.get_embedding_tensor().get_local_tensor()[0]
    changed = float((after != before).any(dim=1).float().mean())
    model.eval()
    with torch.no_grad():
        ids = torch.arange(0, n, 4, device="cuda")
        final = model(ids)
        acc = float((final.argmax(1) == labels[ids]).float().mean())
    final = final.clone()
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
    return losses, acc, changed, final


def test_two_layer_gatv2_model_trains_end_to_end_and_reproducibly(gpu_env):
    import torch
    losses, acc, changed, final = _train_gatv2(gpu_env, 1)
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print("loss %.3f -> %.3f, accuracy %.3f" % (first, last, acc))
    assert np.isfinite(losses).all()
    assert last < 0.6 * first, "loss %.3f -> %.3f" % (first, last)
    assert changed > 0.2, "gradients did not reach the WholeMemory embedding"
    assert acc > 0.7
    losses2, _, _, final2 = _train_gatv2(gpu_env, 1)
    assert losses2 == losses
    assert torch.equal(final.view(torch.int32), final2.view(torch.int32))
