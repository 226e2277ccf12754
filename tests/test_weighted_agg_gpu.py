"""Edge-weighted neighbour aggregation on the MI355X (wholegraph_amd/torch/weighted_aggregation.py ->
csrc/kernels/agg_weighted.hip) and what stands on it: EdgeWeightedSAGEConv and
GraphStructure.multilayer_sample_with_edge_attributes.

Forward, grad_x and grad_w are checked BIT FOR BIT against a numpy restatement written from the header
(include/wholememory/wholegraph_amd_ext.h, section 2d): fp32 scalar operations in the stated order, every product rounded
before the add that follows it, the balanced tree of adjacent pairs over Fp columns for grad_w. No tolerance anywhere: the
order is stated, so the expected bits are derivable."""
import numpy as np
import pytest

import _long_runs as LR

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---------------------------------------------------------------- the order of (2d), restated
def ref_forward(row_ptr, col, terms, x, aggr):
    """terms[e] = fl(w[e] * x[col[e]]) (handed in, so that a caller can form them another way); S(d) left to right from the
    first term; MEAN: S * fl(1 / deg); no edge: +0.0; then x[d]"""
    row_ptr = np.asarray(row_ptr, np.int64)
    n_dst, dim = len(row_ptr) - 1, x.shape[1]
    deg = np.diff(row_ptr)
    acc = np.zeros((n_dst, dim), F32)
    for k in range(int(deg.max()) if n_dst else 0):
        live = np.nonzero(deg > k)[0]
        term = terms[row_ptr[live] + k]
        acc[live] = term if k == 0 else acc[live] + term
    if aggr == "mean":
        nz = deg > 0
        acc[nz] = acc[nz] * (F32(1.0) / deg[nz].astype(F32))[:, None]
    acc[deg == 0] = F32(0.0)
    return np.concatenate([acc, x[:n_dst]], axis=1)


def edge_t(row_ptr, grad_out, aggr):
    """t(e) = grad_out[dst(e), 0:dim], times fl(1 / deg(dst(e))) for MEAN"""
    row_ptr = np.asarray(row_ptr, np.int64)
    n_dst, dim = len(row_ptr) - 1, grad_out.shape[1] // 2
    deg = np.diff(row_ptr)
    dst = np.repeat(np.arange(n_dst), deg)
    t = grad_out[dst, :dim]
    if aggr == "mean":
        t = t * (F32(1.0) / deg[dst].astype(F32))[:, None]
    return t


def ref_grad_x(row_ptr, col, u, grad_out, n_src, chunk):
    """u[e] = fl(w[e] * t(e)) (handed in); P(s) over the edges of s in ascending position, chunks of `chunk` summed left to
    right and added in chunk order; the self term last"""
    col = np.asarray(col, np.int64)
    n_dst, dim = len(row_ptr) - 1, grad_out.shape[1] // 2
    gx = np.zeros((n_src, dim), F32)
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(n_src + 1))
    for s in range(n_src):
        edges = order[starts[s]:starts[s + 1]]
        p = None
        for c0 in range(0, len(edges), chunk):
            part = u[edges[c0]].copy()
            for e in edges[c0 + 1:c0 + chunk]:
                part = part + u[e]
            p = part if p is None else p + part
        if s < n_dst:
            gx[s] = grad_out[s, dim:] if p is None else p + grad_out[s, dim:]
        elif p is not None:
            gx[s] = p
    return gx


def ref_grad_w(col, t, x):
    """q[c] = fl(t(e)[c] * x[col[e], c]), padded with +0.0 to the next power of two, summed as a balanced binary tree of
    adjacent pairs, level by level"""
    dim = x.shape[1]
    fp = 1
    while fp < dim:
        fp *= 2
    q = np.zeros((len(col), fp), F32)
    q[:, :dim] = t * x[np.asarray(col, np.int64)]
    while q.shape[1] > 1:
        q = q[:, 0::2] + q[:, 1::2]
    return q[:, 0].copy()


def ref_all(row_ptr, col, w, x, g, aggr, chunk):
    col64 = np.asarray(col, np.int64)
    t = edge_t(row_ptr, g, aggr)
    out = ref_forward(row_ptr, col, w[:, None] * x[col64], x, aggr)
    gx = ref_grad_x(row_ptr, col, w[:, None] * t, g, x.shape[0], chunk)
    return out, gx, ref_grad_w(col, t, x)


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
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def run_op(x_np, row_ptr, col, w_np, g_np, aggr, want_x=True, want_w=True, x_dev=None):
    """forward + backward on the device -> (out, grad_x or None, grad_w or None) as tensors"""
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    x = (dev(x_np) if x_dev is None else x_dev).detach().requires_grad_(want_x)
    w = dev(w_np).requires_grad_(want_w)
    out = agg_concat_weighted(x, dev(row_ptr), dev(col), w, aggr)
    if want_x or want_w:
        out.backward(dev(g_np))
    return out.detach(), x.grad, w.grad


def check_bitwise(x_np, row_ptr, col, w_np, g_np, aggr, x_dev=None):
    from wholegraph_amd.torch.aggregation import chunk_edges
    out, gx, gw = run_op(x_np, row_ptr, col, w_np, g_np, aggr, x_dev=x_dev)
    want_out, want_gx, want_gw = ref_all(row_ptr, col, w_np, x_np, g_np, aggr, chunk_edges())
    assert out.shape == want_out.shape and gx.shape == want_gx.shape and gw.shape == want_gw.shape
    assert np.array_equal(bits(out), bits(want_out)), "forward"
    assert np.array_equal(bits(gx), bits(want_gx)), "grad_x"
    assert np.array_equal(bits(gw), bits(want_gw)), "grad_w"
    return out, gx, gw


# ---------------------------------------------------------------- 1 bitwise against the restatement
@pytest.mark.parametrize("dim", [1, 3, 4, 33, 100, 128, 256])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_bitwise_power_law_block_with_chunked_hub(gpu_env, dim, aggr):
    """a hub several chunks long (the chunked path and the chunk-order combine), targets without edges, sources without
    edges (targets and others); int64 indices give the same bits"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    C = chunk_edges()
    rng = np.random.default_rng(300 + dim)
    n_dst, n_src = 300, 1200
    row_ptr, col = block(rng, n_dst, n_src, 64, hub=7, hub_share=0.45)
    col[rng.random(len(col)) < 0.1] = 950      # a second hub, not a target
    counts = np.bincount(col, minlength=n_src)
    assert counts[7] > 3 * C, "the hub must exceed C by several chunks"
    assert (np.diff(row_ptr) == 0).any() and (counts[:n_dst] == 0).any() and (counts[n_dst:] == 0).any()
    x = rng.standard_normal((n_src, dim)).astype(F32)
    w = rng.standard_normal(len(col)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    g[5, dim:] = -0.0
    out, gx, gw = check_bitwise(x, row_ptr, col, w, g, aggr)
    xd, wd = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
    out64 = agg_concat_weighted(xd, dev(row_ptr.astype(np.int64)), dev(col.astype(np.int64)), wd, aggr)
    out64.backward(dev(g))
    assert np.array_equal(bits(out64), bits(out)) and np.array_equal(bits(xd.grad), bits(gx))
    assert np.array_equal(bits(wd.grad), bits(gw))


@pytest.mark.parametrize("dim", [3, 128])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_bitwise_uniform_block(gpu_env, dim, aggr):
    rng = np.random.default_rng(17 + dim)
    n_dst, n_src, fan = 500, 3000, 10
    row_ptr = (np.arange(n_dst + 1) * fan).astype(np.int32)
    col = rng.integers(0, n_src, n_dst * fan).astype(np.int32)
    x = rng.standard_normal((n_src, dim)).astype(F32)
    w = rng.random(len(col)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    check_bitwise(x, row_ptr, col, w, g, aggr)


@pytest.mark.parametrize("dim", [3, 128])
def test_bitwise_strided_misaligned_x(gpu_env, dim):
    """a view with a row stride of its own that starts 4 floats into a row of dim + 9: the element-wise route"""
    rng = np.random.default_rng(11)
    n_dst, n_src = 97, 400
    row_ptr, col = block(rng, n_dst, n_src, 40)
    wide = rng.standard_normal((n_src, dim + 9)).astype(F32)
    xv = dev(wide)[:, 4:4 + dim]
    assert xv.stride(0) == dim + 9 and not xv.is_contiguous()
    w = rng.standard_normal(len(col)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    for aggr in ("mean", "sum"):
        check_bitwise(wide[:, 4:4 + dim].copy(), row_ptr, col, w, g, aggr, x_dev=xv)


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_empty_blocks(gpu_env, aggr):
    """E = 0: out = (+0.0, x[d]), grad_x = (the self term for s < n_dst, +0.0 after), grad_w has no entry. n_dst = 0: out has
    no row and grad_x is +0.0"""
    rng = np.random.default_rng(2)
    n_src, dim = 50, 12
    x = rng.standard_normal((n_src, dim)).astype(F32)
    none_i, none_f = np.zeros(0, np.int32), np.zeros(0, F32)
    g = rng.standard_normal((5, 2 * dim)).astype(F32)
    out, gx, gw = check_bitwise(x, np.zeros(6, np.int32), none_i, none_f, g, aggr)
    assert not bits(out[:, :dim]).any() and np.array_equal(bits(out[:, dim:]), bits(x[:5]))
    assert np.array_equal(bits(gx[:5]), bits(g[:, dim:])) and not bits(gx[5:]).any()
    assert gw.shape == (0,)
    out, gx, gw = check_bitwise(x, np.zeros(1, np.int32), none_i, none_f, np.zeros((0, 2 * dim), F32), aggr)
    assert out.shape == (0, 2 * dim) and gx.shape == (n_src, dim) and not bits(gx).any() and gw.shape == (0,)


# ---------------------------------------------------------------- 2 identities with the shipped op
@pytest.mark.parametrize("dim", [3, 128])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_unit_weights_give_agg_concat(gpu_env, dim, aggr):
    from wholegraph_amd.torch.aggregation import agg_concat
    rng = np.random.default_rng(41)
    n_dst, n_src = 300, 1200
    row_ptr, col = block(rng, n_dst, n_src, 64, hub=7, hub_share=0.45)
    x = rng.standard_normal((n_src, dim)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    out, gx, _ = run_op(x, row_ptr, col, np.ones(len(col), F32), g, aggr, want_w=False)
    xd = dev(x).requires_grad_(True)
    plain = agg_concat(xd, dev(row_ptr), dev(col), aggr)
    plain.backward(dev(g))
    assert np.array_equal(bits(out), bits(plain)) and np.array_equal(bits(gx), bits(xd.grad))


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_power_of_two_weights_scale_exactly(gpu_env, aggr):
    """w = +-2^k: every product is exact, so the expected terms are formed by ldexp and a sign, with no multiply at all"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(43)
    n_dst, n_src, dim = 200, 900, 36
    row_ptr, col = block(rng, n_dst, n_src, 48, hub=3, hub_share=0.5)
    col64 = col.astype(np.int64)
    k = rng.integers(-20, 21, len(col))
    sign = np.where(rng.random(len(col)) < 0.5, -1.0, 1.0).astype(F32)
    w = (sign * np.ldexp(F32(1.0), k)).astype(F32)
    x = rng.standard_normal((n_src, dim)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    out, gx, _ = run_op(x, row_ptr, col, w, g, aggr, want_w=False)
    scale = lambda rows: (sign[:, None] * np.ldexp(rows, k[:, None])).astype(F32)   # (exact: far from over- and underflow)
    want_out = ref_forward(row_ptr, col, scale(x[col64]), x, aggr)
    want_gx = ref_grad_x(row_ptr, col, scale(edge_t(row_ptr, g, aggr)), g, n_src, chunk_edges())
    assert np.array_equal(bits(out), bits(want_out)) and np.array_equal(bits(gx), bits(want_gx))


# ---------------------------------------------------------------- 3 hand-derived bits
def test_products_round_before_the_add(gpu_env):
    """a = 1 + 2^-12: a * a = 1 + 2^-11 + 2^-24 exactly, a tie that rounds to even, b = 1 + 2^-11. -b + fl(a * a) is +0.0;
    a fused multiply-add would leave 2^-24. The same pair in the forward sum, in grad_x and in the tree of grad_w."""
    a, b = F32(1.0) + F32(2.0 ** -12), F32(1.0) + F32(2.0 ** -11)
    assert F32(a * a) == b and float(a) * float(a) != float(b)
    # forward: target 0 has the edges (src 1, w = -1) and (src 2, w = a); x[1] = b, x[2] = a
    row_ptr, col = np.array([0, 2], np.int32), np.array([1, 2], np.int32)
    x = np.array([[0.0], [b], [a]], F32)
    w = np.array([-1.0, a], F32)
    g = np.array([[1.0, 0.0]], F32)
    out, _, _ = run_op(x, row_ptr, col, w, g, "sum")
    assert bits(out)[0, 0] == 0x00000000
    # grad_x: source 2 is read by target 0 (w = -1, grad b) and by target 1 (w = a, grad a)
    row_ptr, col = np.array([0, 1, 2], np.int32), np.array([2, 2], np.int32)
    x = np.zeros((3, 1), F32)
    g = np.array([[b, 0.0], [a, 0.0]], F32)
    _, gx, _ = run_op(x, row_ptr, col, np.array([-1.0, a], F32), g, "sum")
    assert bits(gx)[2, 0] == 0x00000000
    # grad_w, dim 2: q = (-1 * b, a * a) -> q0 + q1
    row_ptr, col = np.array([0, 1], np.int32), np.array([1], np.int32)
    x = np.array([[0.0, 0.0], [b, a]], F32)
    g = np.array([[-1.0, a, 0.0, 0.0]], F32)
    _, _, gw = run_op(x, row_ptr, col, np.array([1.0], F32), g, "sum")
    assert bits(gw)[0] == 0x00000000


def test_signed_zeros_nan_and_tree_padding(gpu_env):
    NEG0 = 0x80000000
    # -0.0 terms: the sum starts from its first term, so (-0.0) + (-0.0) stays -0.0, for SUM and (times 1/2) for MEAN
    row_ptr, col = np.array([0, 2, 2], np.int32), np.array([2, 3], np.int32)
    x = np.array([[1.0, 1.0], [1.0, 1.0], [0.0, -0.0], [-0.0, 0.0]], F32)
    w = np.array([-1.0, 1.0], F32)            # terms (-0.0, +0.0) and (-0.0, +0.0)
    g = np.zeros((2, 4), F32)
    for aggr in ("sum", "mean"):
        out, _, _ = run_op(x, row_ptr, col, w, g, aggr)
        assert bits(out)[0, :2].tolist() == [NEG0, 0x00000000]
        assert bits(out)[1, :2].tolist() == [0, 0]            # no edge: +0.0
    # a weight of 0.0 against an inf row is NaN (IEEE), not a skipped edge
    x2 = x.copy()
    x2[2, 0] = np.inf
    out, _, _ = run_op(x2, row_ptr, col, np.array([0.0, 1.0], F32), g, "sum")
    assert np.isnan(out.cpu().numpy()[0, 0]) and bits(out)[0, 1] == 0
    # the tree of grad_w: dim 3 is padded with +0.0, so three -0.0 products give ((-0) + (-0)) + ((-0) + (+0)) = +0.0 (a plain
    # left-to-right chain would keep -0.0); dim 4 has no padding: -0.0
    for dim, want in ((3, 0x00000000), (4, NEG0), (1, NEG0), (2, NEG0)):
        row_ptr, col = np.array([0, 1], np.int32), np.array([1], np.int32)
        x = np.zeros((2, dim), F32)
        x[1] = -0.0
        g = np.ones((1, 2 * dim), F32)                       # q = 1 * -0.0 = -0.0 in every column
        _, _, gw = run_op(x, row_ptr, col, np.array([1.0], F32), g, "sum")
        assert bits(gw)[0] == want, dim


# ---------------------------------------------------------------- 4 determinism; only the gradients asked for
def test_two_calls_give_identical_bits_and_unneeded_gradients_are_not_computed(gpu_env):
    import torch
    from wholegraph_amd.torch import weighted_aggregation as wa
    rng = np.random.default_rng(5)
    n_dst, n_src, fan, dim = 20000, 120000, 30, 128
    row_ptr = (np.arange(n_dst + 1) * fan).astype(np.int32)
    col = (np.minimum(rng.zipf(1.3, n_dst * fan), n_src) - 1).astype(np.int32)
    assert np.bincount(col).max() > 4000
    x = rng.standard_normal((n_src, dim)).astype(F32)
    w = rng.standard_normal(len(col)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    runs = [run_op(x, row_ptr, col, w, g, "mean") for _ in range(2)]
    assert wa.backward_requests[-1] == (True, True)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    out, gx, gw = runs[0]
    # weights without requires_grad: grad_w is passed as a null pointer; the other gradient keeps its bits
    n = len(wa.backward_requests)
    _, gx2, gw2 = run_op(x, row_ptr, col, w, g, "mean", want_w=False)
    assert gw2 is None and wa.backward_requests[-1] == (True, False) and len(wa.backward_requests) == n + 1
    assert torch.equal(gx2.view(torch.int32), gx.view(torch.int32))
    _, gx3, gw3 = run_op(x, row_ptr, col, w, g, "mean", want_x=False)
    assert gx3 is None and wa.backward_requests[-1] == (False, True)
    assert torch.equal(gw3.view(torch.int32), gw.view(torch.int32))
    # ... and at the C entry point: a null grad_w leaves a poisoned buffer next to the call untouched, both null is refused
    import ctypes as C
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import get_stream, get_wholegraph_env_fns
    rp, ci, xd, wd, gd = dev(row_ptr), dev(col), dev(x), dev(w), dev(g)
    gxd = torch.full((n_src, dim), 7.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    call = lambda gx_, gw_: wmb.lib().wholememory_ext_csc_aggregate_weighted_backward(
        p(rp), p(ci), len(col), n_dst, n_src, p(xd), dim, p(wd), p(gd), 2 * dim, dim, wmb.AGGR_MEAN, p(gx_), dim, p(gw_),
        get_wholegraph_env_fns(), C.c_void_p(get_stream()))
    assert call(None, None) == 6   # WHOLEMEMORY_INVALID_INPUT
    gwd = torch.full((len(col),), 7.0, device="cuda")
    assert call(None, gwd) == 0
    torch.cuda.synchronize()
    assert bool((gxd == 7.0).all()) and torch.equal(gwd.view(torch.int32), gw.view(torch.int32))
    gwd.fill_(7.0)
    assert call(gxd, None) == 0
    torch.cuda.synchronize()
    assert bool((gwd == 7.0).all()) and torch.equal(gxd.view(torch.int32), gx.view(torch.int32))


@pytest.mark.parametrize("dim", [5, 8])
def test_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, dim):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third.
    (It stands behind the test above, which counts the entries of the op's capped log of backward calls.)"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(900 + dim)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    x = rng.standard_normal((LR.N_SRC, dim)).astype(F32)
    w = rng.standard_normal(len(col)).astype(F32)
    g = rng.standard_normal((LR.N_DST, 2 * dim)).astype(F32)
    for aggr in ("mean", "sum"):
        check_bitwise(x, row_ptr, col, w, g, aggr)


# ---------------------------------------------------------------- 5 the layer
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("root_weight,project,normalize,bias", [(True, False, False, True), (False, False, False, True),
                                                                (True, True, False, True), (True, False, True, False),
                                                                (False, True, True, False)])
def test_layer_is_linear_of_the_op(gpu_env, aggr, root_weight, project, normalize, bias):
    import torch
    import torch.nn.functional as Fn
    from wholegraph_amd.torch.cugraphops import EdgeWeightedSAGEConv
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout = 150, 700, 48, 24
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    layer = EdgeWeightedSAGEConv(cin, cout, aggr=aggr, root_weight=root_weight, project=project, normalize=normalize,
                                 bias=bias).cuda()
    assert (layer.lin.bias is not None) == bias
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    w = dev(rng.random(len(col)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, 20, w)
    assert out.shape == (n_dst, cout)
    h = layer.pre_lin(x).relu() if project else x
    cat = agg_concat_weighted(h, rp, ci, w, aggr)
    want = layer.lin(cat if root_weight else cat[:, :cin])
    if normalize:
        want = Fn.normalize(want, p=2.0, dim=-1)
    assert torch.equal(out, want)
    out.square().sum().backward()
    params = dict(layer.named_parameters())
    assert "lin.weight" in params and (("pre_lin.weight" in params) == project)
    for name, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
    assert x.grad is not None and x.grad.abs().sum() > 0 and w.grad is not None and w.grad.abs().sum() > 0


def test_layer_under_autocast_and_16_bit_rows_outside_it(gpu_env):
    import torch
    from wholegraph_amd.torch.cugraphops import EdgeWeightedSAGEConv
    from wholegraph_amd.torch.weighted_aggregation import agg_concat_weighted
    torch.manual_seed(0)
    rng = np.random.default_rng(22)
    n_dst, n_src, cin = 120, 500, 32
    row_ptr, col = block(rng, n_dst, n_src, 16)
    rp, ci = dev(row_ptr), dev(col)
    w = dev(rng.random(len(col)).astype(F32)).requires_grad_(True)
    x16 = dev(rng.standard_normal((n_src, cin)).astype(F32)).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = agg_concat_weighted(x16, rp, ci, w, "mean")
    assert got.dtype == torch.float32
    assert torch.equal(got, agg_concat_weighted(x16.float(), rp, ci, w, "mean"))
    layer = EdgeWeightedSAGEConv(cin, 8, project=True).cuda()
    x = x16.float().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, rp, ci, 16, w)          # pre_lin hands the op bf16 rows
        h = layer.pre_lin(x).relu()
        assert h.dtype == torch.bfloat16
        want = layer.lin(agg_concat_weighted(h.float(), rp, ci, w, "mean"))
    assert out.dtype == torch.bfloat16 and torch.equal(out, want)
    out.float().sum().backward()
    assert x.grad is not None and w.grad is not None and torch.isfinite(w.grad).all() and w.grad.abs().sum() > 0
    for bad in (x16, x16.half()):
        with pytest.raises(TypeError, match="float32"):
            agg_concat_weighted(bad, rp, ci, w, "mean")


# ---------------------------------------------------------------- 6 the sampler helper
def _wm_array(comm, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


def _weighted_graph(comm, n_nodes, max_deg, seed, heavy=()):
    import wholegraph_amd.torch as wgth
    from test_graph_oracle import make_csr
    row_ptr, col = make_csr(n_nodes, max_deg, seed, np.int64, heavy=list(heavy))
    rng = np.random.default_rng(seed + 1)
    weights = (rng.random(len(col)) + 0.1).astype(F32)
    tag = rng.integers(0, 1 << 30, len(col)).astype(np.int64)
    ts = [_wm_array(comm, a) for a in (row_ptr, col, weights, tag)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("w", ts[2])
    g.set_edge_attribute("tag", ts[3])
    return g, ts, row_ptr, col, weights, tag


@pytest.mark.parametrize("weight_name", [None, "w"])
def test_sampler_helper_delivers_the_attributes_of_the_sampled_edges(gpu_env, weight_name):
    import torch
    import wholegraph_amd.torch as wgth
    n_nodes = 20011
    g, ts, row_ptr, col, weights, tag = _weighted_graph(gpu_env, n_nodes, 70, 41, heavy=[(3, 4000), (4, 0)])
    seeds = torch.from_numpy(np.random.default_rng(3).permutation(n_nodes)[:512].astype(np.int64)).cuda()
    seeds[:2] = torch.tensor([3, 4])
    fan, rs = [30, 10], [7, 8]
    plain = g.multilayer_sample_without_replacement(seeds, fan, weight_name, random_seeds=rs)
    got = g.multilayer_sample_with_edge_attributes(seeds, fan, ["w", "tag", "__edge_id__"], weight_name, random_seeds=rs)
    assert len(got) == 5
    for a_list, b_list in zip(plain, got[:4]):
        assert len(a_list) == len(b_list)
        for a, b in zip(a_list, b_list):
            assert a.dtype == b.dtype and torch.equal(a, b)
    target_gids, edge_indice, csr_row_ptr, csr_col_ind, attrs = got
    assert len(attrs) == len(fan)
    for layer in range(len(fan)):
        assert sorted(attrs[layer]) == ["__edge_id__", "tag", "w"]
        eid = attrs[layer]["__edge_id__"].cpu().numpy()
        n_edges = csr_col_ind[layer].numel()
        assert eid.dtype == np.int64 and eid.shape == (n_edges,)
        assert attrs[layer]["w"].dtype == torch.float32 and attrs[layer]["tag"].dtype == torch.int64
        gids = target_gids[layer].cpu().numpy()
        rp = csr_row_ptr[layer].cpu().numpy().astype(np.int64)
        centre = gids[np.repeat(np.arange(len(rp) - 1), np.diff(rp))]        # global id of every block edge's centre
        src = gids[csr_col_ind[layer].cpu().numpy()]                         # ... and of its source position
        assert np.all((eid >= row_ptr[centre]) & (eid < row_ptr[centre + 1])), "edge id outside its centre's CSR row"
        assert np.array_equal(col[eid], src), "the graph edge does not lead to the block edge's source"
        assert np.array_equal(attrs[layer]["w"].cpu().numpy().view(np.uint32), weights[eid].view(np.uint32))
        assert np.array_equal(attrs[layer]["tag"].cpu().numpy(), tag[eid])
    with pytest.raises(AssertionError):
        g.multilayer_sample_with_edge_attributes(seeds, fan, ["nope"], weight_name, random_seeds=rs)
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


# ---------------------------------------------------------------- 7 end to end
def _train(comm, g, n_edges, n_nodes, feats, labels):
    import torch
    import torch.nn.functional as Fn
    from wholegraph_amd.torch.cugraphops import EdgeWeightedSAGEConv
    torch.manual_seed(1)
    rng = np.random.default_rng(2)
    l1, l2 = EdgeWeightedSAGEConv(feats.shape[1], 32).cuda(), EdgeWeightedSAGEConv(32, int(labels.max()) + 1).cuda()
    theta = torch.nn.Parameter(torch.ones(n_edges, device="cuda"))       # a learnable gate per graph edge
    params = list(l1.parameters()) + list(l2.parameters()) + [theta]
    opt = torch.optim.SGD(params, lr=0.05)
    for step in range(20):
        ids = torch.from_numpy(rng.choice(n_nodes, 128, replace=False).astype(np.int64)).cuda()
        gids, _, rps, cis, attrs = g.multilayer_sample_with_edge_attributes(ids, [8, 8], ["__edge_id__"], "w",
                                                                           random_seeds=[100 + step, 200 + step])
        h = feats[gids[0]]
        h = l1(h, rps[0], cis[0], 8, theta[attrs[0]["__edge_id__"]]).relu()
        logits = l2(h, rps[1], cis[1], 8, theta[attrs[1]["__edge_id__"]])
        loss = Fn.cross_entropy(logits, labels[ids])
        opt.zero_grad()
        loss.backward()
        assert theta.grad is not None and theta.grad.abs().sum() > 0, "no gradient reached the edge weights"
        opt.step()
    assert torch.isfinite(loss)
    return [p.detach().clone() for p in params]


def test_two_layers_train_deterministically_with_learnable_edge_weights(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    n_nodes = 3000
    g, ts, row_ptr, col, weights, tag = _weighted_graph(gpu_env, n_nodes, 24, 77, heavy=[(5, 900)])
    rng = np.random.default_rng(9)
    feats = dev(rng.standard_normal((n_nodes, 16)).astype(F32))
    labels = dev(rng.integers(0, 4, n_nodes).astype(np.int64))
    a = _train(gpu_env, g, len(col), n_nodes, feats, labels)
    b = _train(gpu_env, g, len(col), n_nodes, feats, labels)
    assert len(a) == len(b) and len(a) >= 5
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    assert bool((a[-1] != 1.0).any()), "the edge gates did not move"
    for t in ts:
        wgth.destroy_wholememory_tensor(t)
