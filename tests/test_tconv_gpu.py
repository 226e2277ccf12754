"""Scaled dot-product attention aggregation on the MI355X (wholegraph_amd/torch/transformer_aggregation.py ->
csrc/kernels/tconv.hip).

The logits are restated bit for bit (tree and scale included) and alpha is checked against a float64 softmax of them; out
and the three gradients are checked bit for bit against a numpy restatement of the order the header states
(include/wholememory/wholegraph_amd_ext.h, section 2k), fed the op's own alpha, and with allclose against torch autograd
through an index_select / scatter-amax / index_add_ composite (rtol 1e-5 for out, 1e-4 for gradients: the tolerances the GAT
tests take; on the hub block the restatement against float64 uses at most 0.12 of the first and 0.02 of the second). Then
TransformerConv against the composite, and a two-layer "transformer" HomoGNNModel trained end to end on a planted-partition
graph held in WholeMemory."""
import random
import types

import numpy as np
import pytest

import _long_runs as LR
from test_gat_gpu import assert_close_scaled, edge_dst, ref_out, seg_sum
from test_gatv2_gpu import hub_block, ref_alpha64, tree_sum
from test_sage_agg_gpu import _planted_partition, _wm_array, bits, block, dev

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (2, 3), (3, 4), (4, 8), (4, 32), (2, 128), (8, 64), (1, 256), (1, 512)]


# ---------------------------------------------------------------- the order, restated
def scale_of(F):
    """fl(1.0f / fl(sqrtf((float)F)))"""
    return F32(1.0) / np.sqrt(F32(F))


def ref_logits(row_ptr, col, key, query, H, norm):
    F = key.shape[1] // H
    dst = edge_dst(row_ptr)
    t = tree_sum(query[dst].reshape(-1, H, F) * key[np.asarray(col, np.int64)].reshape(-1, H, F))
    return (t * scale_of(F)).astype(F32) if norm else t


def per_source(col, n_src, terms, chunk):
    """per source, the sum of its edges' terms in ascending edge position: left to right within chunks of `chunk` edges, the
    chunk sums added in chunk order; +0.0 for a source without edges"""
    out = np.zeros((n_src,) + terms.shape[1:], F32)
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
        out[j] = p
    return out


def ref_backward(row_ptr, col, key, query, value, alpha, G, H, concat, norm, chunk):
    """(grad_key, grad_query, grad_value) in the stated order, from the op's alpha"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, n_src, hf = len(row_ptr) - 1, key.shape[0], key.shape[1]
    F = hf // H
    Gk = G.reshape(n_dst, H, F) if concat else np.broadcast_to(G[:, None, :] * (F32(1.0) / F32(H)), (n_dst, H, F))
    dst = edge_dst(row_ptr)
    da = tree_sum(Gk[dst] * value[col].reshape(-1, H, F))
    c = seg_sum(row_ptr, alpha * da)
    dl = (alpha * (da - c[dst])).astype(F32)
    ds = (dl * scale_of(F)).astype(F32) if norm else dl
    gq = seg_sum(row_ptr, ds[:, :, None] * key[col].reshape(-1, H, F))
    gk = per_source(col, n_src, ds[:, :, None] * query[dst].reshape(-1, H, F), chunk)
    gv = per_source(col, n_src, alpha[:, :, None] * Gk[dst], chunk)
    return gk.reshape(n_src, hf), gq.reshape(n_dst, hf), gv.reshape(n_src, hf)


def composite(key, query, value, row_ptr, col, H, concat, norm):
    """torch autograd reference: index_select, a scatter-amax / exp / index_add_ softmax, index_add_"""
    import torch
    n_dst = row_ptr.numel() - 1
    F = key.shape[1] // H
    kv, qv, vv = key.view(-1, H, F), query.view(-1, H, F), value.view(-1, H, F)
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=key.device), deg)
    col = col.long()
    l = (qv[dst] * kv[col]).sum(-1)
    if norm:
        l = l / float(np.sqrt(F))
    m = torch.full((n_dst, H), -float("inf"), device=key.device, dtype=key.dtype).scatter_reduce(
        0, dst[:, None].expand(-1, H), l.detach(), "amax", include_self=True)
    w = torch.exp(l - m[dst])
    den = torch.zeros((n_dst, H), device=key.device, dtype=key.dtype).index_add_(0, dst, w)
    alpha = w / den[dst]
    o = torch.zeros((n_dst, H, F), device=key.device, dtype=key.dtype).index_add_(0, dst, alpha[:, :, None] * vv[col])
    return o.reshape(n_dst, H * F) if concat else o.mean(1)


def inputs(rng, n_src, n_q, H, F):
    """key, query and value: three different random arrays"""
    return (rng.standard_normal((n_src, H * F)).astype(F32), rng.standard_normal((n_q, H * F)).astype(F32),
            rng.standard_normal((n_src, H * F)).astype(F32))


def run_op(k_t, q_t, v_t, row_ptr, col, G_np, H, concat, norm, need=(True, True, True), index=np.int32):
    """(out, alpha, grads) of one forward + backward; grads[i] is None where need[i] is False"""
    from wholegraph_amd.torch.transformer_aggregation import mha_simple_n2n
    k, q, v = (t.detach().requires_grad_(n) for t, n in zip((k_t, q_t, v_t), need))
    out, alpha = mha_simple_n2n(k, q, v, dev(np.asarray(row_ptr, index)), dev(np.asarray(col, index)), H, concat, norm,
                                return_alpha=True)
    out.backward(dev(G_np))
    return out.detach(), alpha.detach(), [t.grad for t in (k, q, v)]


def check_all(k_np, q_np, v_np, row_ptr, col, H, concat, norm, rng, tensors=None, loose=True):
    """every output of the op against the restatement (alpha within its bound, the rest bit for bit) and, with `loose`,
    against torch autograd through the composite; returns the op's outputs"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    n_dst, hf = len(row_ptr) - 1, k_np.shape[1]
    G_np = rng.standard_normal((n_dst, hf if concat else hf // H)).astype(F32)
    k_t, q_t, v_t = (dev(k_np), dev(q_np), dev(v_np)) if tensors is None else tensors
    out, alpha, grads = run_op(k_t, q_t, v_t, row_ptr, col, G_np, H, concat, norm)
    assert out.shape == ((n_dst, hf) if concat else (n_dst, hf // H)) and alpha.shape == (len(col), H)
    al = alpha.cpu().numpy()
    l32 = ref_logits(row_ptr, col, k_np, q_np[:n_dst], H, norm)
    ref, bound = ref_alpha64(row_ptr, l32)
    print("alpha: max |err| / bound = %.3g" % (float(np.max(np.abs(al - ref) / bound)) if len(col) else 0.0))
    assert (np.abs(al - ref) <= bound).all(), "alpha off by %g" % float(np.max(np.abs(al - ref) / (ref + 1e-30)))
    assert np.array_equal(bits(out), ref_out(row_ptr, col, v_np, al, H, concat).view(np.uint32)), "out"
    gk, gq, gv = ref_backward(row_ptr, col, k_np, q_np[:n_dst], v_np, al, G_np, H, concat, norm, chunk_edges())
    assert np.array_equal(bits(grads[0]), gk.view(np.uint32)), "grad_key"
    assert np.array_equal(bits(grads[1])[:n_dst], gq.view(np.uint32)), "grad_query"
    assert not grads[1][n_dst:].any()
    assert np.array_equal(bits(grads[2]), gv.view(np.uint32)), "grad_value"
    if loose:   # the tolerances test_gat_gpu.py takes for the same comparison
        k2, q2, v2 = (dev(a).requires_grad_(True) for a in (k_np, q_np, v_np))
        want = composite(k2, q2, v2, dev(row_ptr), dev(col), H, concat, norm)
        assert_close_scaled(out, want.detach(), 1e-5)
        want.backward(dev(G_np))
        for got, w in zip(grads, (k2.grad, q2.grad, v2.grad)):
            assert_close_scaled(got, w)
    return out, alpha, grads, G_np


# ---------------------------------------------------------------- 1 every lane mapping, forward and backward
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("norm", [True, False])
def test_bitwise_on_hub_block(gpu_env, H, F, concat, norm):
    """Fp = 1, tree padding (F = 3), one lane per head (F = 4), heads sharing a wave, lane groups of 16 / 32 / 64, rows with
    more pieces than lanes (8 x 64), a head that spans a whole wave (F = 256) and F beyond the lane-split tree (512)"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(2000 + 10 * H + F + concat + 2 * norm)
    k, q, v = inputs(rng, n_src, n_dst, H, F)
    check_all(k, q, v, row_ptr, col, H, concat, norm, rng)


# ---------------------------------------------------------------- 2 long runs of partial rows
@pytest.mark.parametrize("F", [5, 8])
def test_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, F):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    C, H = chunk_edges(), 2
    rng = np.random.default_rng(910 + F)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    k, q, v = inputs(rng, LR.N_SRC, LR.N_DST, H, F)
    for concat in (True, False):
        check_all(k, q, v, row_ptr, col, H, concat, True, rng, loose=False)


# ---------------------------------------------------------------- 3 the element-wise path gives the same bits
def test_misaligned_strided_views_equal_the_16_byte_path(gpu_env):
    import torch
    rng = np.random.default_rng(7)
    H, F, n_dst, n_src = 4, 8, 97, 260
    hf = H * F
    row_ptr, col = block(rng, n_dst, n_src, 30)
    wide_k = rng.standard_normal((n_src, hf + 9)).astype(F32)
    wide_q = rng.standard_normal((n_dst + 3, hf + 6)).astype(F32)   # rows behind the targets
    wide_v = rng.standard_normal((n_src, hf + 5)).astype(F32)
    views = tuple(dev(w)[:, 3:3 + hf] for w in (wide_k, wide_q, wide_v))   # offset 3 floats: not 16-byte aligned
    assert all(not t.is_contiguous() and t.data_ptr() % 16 for t in views)
    assert len({t.stride(0) for t in views}) == 3
    k, q, v = (w[:, 3:3 + hf].copy() for w in (wide_k, wide_q, wide_v))
    for concat in (True, False):
        out, alpha, grads, G = check_all(k, q, v, row_ptr, col, H, concat, True, np.random.default_rng(8), tensors=views,
                                         loose=False)
        assert grads[1].shape[0] == n_dst + 3 and not grads[1][n_dst:].any()
        out2, alpha2, grads2 = run_op(dev(k), dev(q), dev(v), row_ptr, col, G, H, concat, True)   # aligned: lane-split tree
        for a, b in zip([out, alpha] + grads, [out2, alpha2] + grads2):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------- 4 self loops, empty blocks, int64 indices
def test_self_loops_from_add_csr_self_loop(gpu_env):
    from wholegraph_amd.torch.graph_ops import add_csr_self_loop
    rng = np.random.default_rng(10)
    H, F, n_dst, n_src = 2, 16, 60, 200
    row_ptr, col = block(rng, n_dst, n_src, 9)
    rp, ci = add_csr_self_loop(dev(row_ptr), dev(col))
    rp_np, ci_np = rp.cpu().numpy(), ci.cpu().numpy()
    assert len(ci_np) == len(col) + n_dst and (np.diff(rp_np) >= 1).all()
    k, q, v = inputs(rng, n_src, n_dst, H, F)
    check_all(k, q, v, rp_np, ci_np, H, False, True, rng)


def test_empty_blocks(gpu_env):
    rng = np.random.default_rng(11)
    H, F, n_src = 2, 8, 50
    for n_dst in (0, 6):   # n_dst = 0, then E = 0 with targets
        k, q, v = inputs(rng, n_src, n_dst, H, F)
        rp = np.zeros(n_dst + 1, np.int32)
        for concat in (True, False):
            out, alpha, grads, _ = check_all(k, q, v, rp, np.zeros(0, np.int32), H, concat, True, rng, loose=False)
            assert not out.any() and all(not g.any() for g in grads)
            assert all(np.array_equal(bits(g), np.zeros(g.shape, np.uint32)) for g in [out] + grads)   # +0.0


def test_int64_indices_give_the_bits_of_int32(gpu_env):
    import torch
    rng = np.random.default_rng(13)
    H, F, n_dst, n_src = 2, 16, 60, 200
    row_ptr, col = block(rng, n_dst, n_src, 9)
    k, q, v = (dev(a) for a in inputs(rng, n_src, n_dst, H, F))
    G = rng.standard_normal((n_dst, H * F)).astype(F32)
    a = run_op(k, q, v, row_ptr, col, G, H, True, True)
    b = run_op(k, q, v, row_ptr, col, G, H, True, True, index=np.int64)
    for x, y in zip(a[:2] + tuple(a[2]), b[:2] + tuple(b[2])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------- 5 large logits
def test_large_logits_stay_finite(gpu_env):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(14)
    H, F = 4, 32
    k, q, v = inputs(rng, n_src, n_dst, H, F)
    k, q = (k * F32(30)).astype(F32), (q * F32(30)).astype(F32)
    out, alpha, grads, _ = check_all(k, q, v, row_ptr, col, H, True, False, rng)
    assert all(bool(torch.isfinite(t).all()) for t in [out, alpha] + grads)
    al = alpha.cpu().numpy().astype(np.float64)
    _, bound = ref_alpha64(row_ptr, ref_logits(row_ptr, col, k, q, H, False))
    dst = edge_dst(row_ptr)
    tot, room = np.zeros((n_dst, H)), np.zeros((n_dst, H))
    np.add.at(tot, dst, al)
    np.add.at(room, dst, bound)
    has = np.diff(row_ptr) > 0
    assert (np.abs(tot[has] - 1.0) <= room[has] + 1e-15).all()


# ---------------------------------------------------------------- 6 reproducibility, gradients on their own
def test_identical_calls_and_single_gradients_give_identical_bits(gpu_env):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(12)
    H, F = 4, 32
    k, q, v = (dev(a) for a in inputs(rng, n_src, n_dst, H, F))
    G = rng.standard_normal((n_dst, H * F)).astype(F32)
    full = run_op(k, q, v, row_ptr, col, G, H, True, True)
    again = run_op(k, q, v, row_ptr, col, G, H, True, True)
    for a, b in zip(full[:2] + tuple(full[2]), again[:2] + tuple(again[2])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for i in range(3):
        need = tuple(j == i for j in range(3))
        _, _, grads = run_op(k, q, v, row_ptr, col, G, H, True, True, need)
        assert [g is not None for g in grads] == list(need)
        assert torch.equal(grads[i].view(torch.int32), full[2][i].view(torch.int32))


# ---------------------------------------------------------------- 7 TransformerConv
def layer_reference(layer, x, rp, ci):
    """the layer's forward with the composite in place of the op; also the key rows it fed the composite"""
    import torch
    n_dst = rp.numel() - 1
    key = layer.lin_key(x)
    out = composite(key, layer.lin_query(x[:n_dst]), layer.lin_value(x), rp, ci, layer.heads, layer.concat, True)
    if layer.root_weight:
        x_r = layer.lin_skip(x[:n_dst])
        if layer.beta:
            b = torch.sigmoid(layer.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)))
            out = b * x_r + (1 - b) * out
        else:
            out = out + x_r
    return out, key


@pytest.mark.parametrize("concat,beta,root", [(True, False, True), (True, True, True), (False, False, True),
                                              (False, True, True), (True, False, False)])
def test_transformer_conv_matches_composite(gpu_env, concat, beta, root):
    """Every gradient is finite, non-zero and close to the composite's — but for lin_key.bias, whose gradient is exactly zero:
    a constant added to every key row moves all logits of a target by the same query . b, which the softmax does not see.
    What either side returns for it is the rounding left over from a sum of terms that cancel (1e-7 here), and a tolerance
    relative to such a value means nothing. Its scale is that of the terms, the rows of the key gradient: both sides must
    be zero within the gradient tolerance (1e-4) of the column sums of their absolute values."""
    import torch
    from wholegraph_amd.torch.cugraphops import TransformerConv
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout, H = 150, 700, 48, 24, 4
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    layer = TransformerConv(cin, cout, heads=H, concat=concat, beta=beta, root_weight=root).cuda()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, 20)
    assert out.shape == ((n_dst, H * cout) if concat else (n_dst, cout))
    x2 = x.detach().clone().requires_grad_(True)
    ref, ref_key = layer_reference(layer, x2, rp, ci)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
    params = dict(layer.named_parameters())
    names = sorted(params)
    assert ("lin_beta.weight" in names) == beta and ("lin_skip.weight" in names) == root
    got = torch.autograd.grad(out.square().sum(), [x] + [params[n] for n in names])
    want = torch.autograd.grad(ref.square().sum(), [x2, ref_key] + [params[n] for n in names])
    key_terms = want[1].double().abs().sum(0)
    for name, g, w in zip(["x"] + names, got, want[:1] + want[2:]):
        assert torch.isfinite(g).all(), name
        if name == "lin_key.bias":
            print("lin_key.bias: max |got| %.3g, |want| %.3g, of terms that sum to %.3g" % (
                float(g.abs().max()), float(w.abs().max()), float(key_terms.min())))
            assert bool((g.double().abs() <= 1e-4 * key_terms).all()) and bool((w.double().abs() <= 1e-4 * key_terms).all())
            continue
        assert g.abs().sum() > 0, name
        assert_close_scaled(g, w)


def test_transformer_conv_under_autocast_and_16_bit_rows_outside_it(gpu_env):
    import torch
    from wholegraph_amd.torch.cugraphops import TransformerConv
    from wholegraph_amd.torch.transformer_aggregation import mha_simple_n2n
    torch.manual_seed(3)
    rng = np.random.default_rng(22)
    n_dst, n_src, cin, cout, H = 80, 300, 32, 16, 2
    row_ptr, col = block(rng, n_dst, n_src, 12)
    rp, ci = dev(row_ptr), dev(col)
    layer = TransformerConv(cin, cout, heads=H).cuda()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        k, q, v = layer.lin_key(x), layer.lin_query(x[:n_dst]), layer.lin_value(x)
        x_r = layer.lin_skip(x[:n_dst])
        assert k.dtype == torch.bfloat16
        out = layer(x, rp, ci, 12)
    assert out.dtype == torch.float32
    # the op saw the bf16 Linear outputs widened to fp32
    want = mha_simple_n2n(k.float(), q.float(), v.float(), rp, ci, H) + x_r
    assert torch.equal(out.detach().view(torch.int32), want.detach().view(torch.int32))
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    k, q, v = k.detach().float(), q.detach().float(), v.detach().float()
    for dt in (torch.float16, torch.bfloat16):
        for i in range(3):
            args = [k, q, v]
            args[i] = args[i].to(dt)
            with pytest.raises(TypeError, match="float32"):
                mha_simple_n2n(*args, rp, ci, H)


# ---------------------------------------------------------------- 8 end to end
def _train_transformer(comm, seed):
    """a 2-layer, 2-head "transformer" HomoGNNModel on the planted-partition graph of the GATv2 end-to-end test: the losses,
    the accuracy, the share of embedding rows that moved and the final evaluation logits"""
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
    args = types.SimpleNamespace(model="transformer", hiddensize=64, layernum=2, classnum=k, dropout=0.1, neighbors="10,10",
                                 inferencesample="10,10", heads=2)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    assert [type(l).__name__ for l in model.gnn_layers] == ["TransformerConv"] * 2 and not model.add_self_loop
    assert [(l.heads, l.concat, l.out_channels) for l in model.gnn_layers] == [(2, True, 32), (2, False, k)]
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


def test_two_layer_transformer_model_trains_end_to_end_and_reproducibly(gpu_env):
    """The bars are those of the GATv2 test. The reference they were checked against: this model with mha_simple_n2n
    replaced by the torch composite above, on the MI355X, gave loss 0.6977 -> 0.0045 (ratio 0.0064), accuracy 0.998 and every
    embedding row moved with seed 1 (the op itself: the same figures to four digits), ratio 0.036 / accuracy 0.999 with seed
    2 and ratio 0.008 / accuracy 1.000 with seed 3: it clears `last < 0.6 * first` and accuracy > 0.7, so they stand."""
    import torch
    losses, acc, changed, final = _train_transformer(gpu_env, 1)
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print("loss %.3f -> %.3f, accuracy %.3f, changed %.3f" % (first, last, acc, changed))
    assert np.isfinite(losses).all()
    assert last < 0.6 * first, "loss %.3f -> %.3f" % (first, last)
    assert changed > 0.2, "gradients did not reach the WholeMemory embedding"
    assert acc > 0.7
    losses2, _, _, final2 = _train_transformer(gpu_env, 1)
    assert losses2 == losses
    assert torch.equal(final.view(torch.int32), final2.view(torch.int32))
