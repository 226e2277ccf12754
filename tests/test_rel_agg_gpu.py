"""Relation-typed neighbour aggregation on the MI355X (wholegraph_amd/torch/rel_aggregation.py -> csrc/kernels/agg_rel.hip)
and what stands on it: RGCNConv and HomoGNNModel(model="rgcn").

Forward, edge_scale and grad_x are checked BIT FOR BIT against a numpy restatement written from the header
(include/wholememory/wholegraph_amd_ext.h, section 2h): fp32 scalar operations in the stated order, every product rounded
before the add that follows it. No tolerance anywhere: the order is stated, so the expected bits are derivable."""
import random
import types

import numpy as np
import pytest

import _long_runs as LR

pytestmark = pytest.mark.gpu

F32 = np.float32
NEG0 = 0x80000000


# ---------------------------------------------------------------- the order of (2h), restated
def ref_forward(row_ptr, col, et, R, x, aggr):
    """per target and relation r: S_r left to right from the first term over the edges of type r in ascending position;
    MEAN: fl(S_r * fl(1 / n_r)); no such edge: +0.0; then x[d]. edge_scale[e] = fl(1 / n_r) of its target and type, +0.0 for a
    type outside [0, R) (such an edge enters nothing)"""
    n_dst, dim = len(row_ptr) - 1, x.shape[1]
    out = np.zeros((n_dst, (R + 1) * dim), F32)
    scale = np.zeros(len(col), F32)
    for d in range(n_dst):
        acc, cnt = {}, {}
        edges = range(int(row_ptr[d]), int(row_ptr[d + 1]))
        for e in edges:
            r = int(et[e])
            if not 0 <= r < R:
                continue
            acc[r] = x[col[e]].copy() if r not in acc else acc[r] + x[col[e]]
            cnt[r] = cnt.get(r, 0) + 1
        for r, a in acc.items():
            out[d, r * dim:(r + 1) * dim] = a * (F32(1.0) / F32(cnt[r])) if aggr == "mean" else a
        for e in edges:
            if 0 <= int(et[e]) < R:
                scale[e] = F32(1.0) / F32(cnt[int(et[e])])
        out[d, R * dim:] = x[d]
    return out, scale


def ref_grad_x(row_ptr, col, et, R, scale, g, n_src, chunk, aggr):
    """u(e) = g[dst(e), slot type(e)] (MEAN: fl(edge_scale[e] * that)); P(s) over the edges of s in ascending position, cut
    into chunks of `chunk` consecutive positions of the run (an edge with a type out of range keeps its position and adds
    nothing), each chunk left to right, the chunk sums added in chunk order; the self term last"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, dim = len(row_ptr) - 1, g.shape[1] // (R + 1)
    dst = np.repeat(np.arange(n_dst), np.diff(row_ptr))
    gx = np.zeros((n_src, dim), F32)
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(n_src + 1))
    for s in range(n_src):
        edges = order[starts[s]:starts[s + 1]]
        p = None
        for c0 in range(0, len(edges), chunk):
            part = None
            for e in edges[c0:c0 + chunk]:
                r = int(et[e])
                if not 0 <= r < R:
                    continue
                u = g[dst[e], r * dim:(r + 1) * dim]
                if aggr == "mean":
                    u = scale[e] * u
                part = u.copy() if part is None else part + u
            if part is not None:
                p = part if p is None else p + part
        if s < n_dst:
            gx[s] = g[s, R * dim:] if p is None else p + g[s, R * dim:]
        elif p is not None:
            gx[s] = p
    return gx


def typed_block(rng, R, n_dst=300, n_src=900, hub=7, hub_share=0.3, hub2=850):
    """a power-law block: degrees 0, 1, the group widths and their successors, 70 (more than a wave); a hub source (a target)
    behind `hub_share` of the edges and a second hub that is no target; types interleaved within a target; relation R - 1
    absent everywhere and relation d % (R - 1) absent from target d (R >= 3); target 3's edges all of type 0"""
    deg = np.floor(70.0 * rng.random(n_dst) ** 3).astype(np.int64)
    deg[:12] = [0, 70, 1, 33, 16, 17, 32, 64, 65, 2, 70, 0]
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    E = int(row_ptr[-1])
    col = rng.integers(0, n_src, E).astype(np.int32)
    col[rng.random(E) < hub_share] = hub
    col[rng.random(E) < 0.05] = hub2
    col[col == 11] = 12                                # a target and a non-target that nobody reads
    col[col == n_src - 1] = n_src - 2
    dst = np.repeat(np.arange(n_dst), deg)
    if R == 1:
        et = np.zeros(E, np.int32)
    else:
        live = R - 1                                   # relation R - 1 has no edge at all
        et = rng.integers(0, live, E).astype(np.int32)
        if live >= 2:
            clash = et == dst % live                   # ... and target d has none of relation d % (R - 1)
            et[clash] = (et[clash] + 1) % live
        et[dst == 3] = 0
    return row_ptr, col, et


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def run_op(x_np, row_ptr, col, et, R, g_np, aggr, x_dev=None, wide_index=False):
    """forward + backward on the device -> (out, edge_scale or None, grad_x) as tensors"""
    from wholegraph_amd.torch.rel_aggregation import agg_concat_rel
    x = (dev(x_np) if x_dev is None else x_dev).detach().requires_grad_(True)
    if wide_index:
        row_ptr, col, et = (np.asarray(a).astype(np.int64) for a in (row_ptr, col, et))
    out = agg_concat_rel(x, dev(row_ptr), dev(col), dev(et), R, aggr)
    scale = out.grad_fn.saved_tensors[3]
    out.backward(dev(g_np))
    return out.detach(), scale, x.grad


def check_bitwise(x_np, row_ptr, col, et, R, g_np, aggr, **kw):
    from wholegraph_amd.torch.aggregation import chunk_edges
    out, scale, gx = run_op(x_np, row_ptr, col, et, R, g_np, aggr, **kw)
    want_out, want_scale = ref_forward(row_ptr, col, et, R, x_np, aggr)
    want_gx = ref_grad_x(row_ptr, col, et, R, want_scale, g_np, x_np.shape[0], chunk_edges(), aggr)
    assert out.shape == want_out.shape and gx.shape == want_gx.shape
    assert np.array_equal(bits(out), bits(want_out)), "forward"
    if aggr == "mean":
        assert scale.shape == want_scale.shape and np.array_equal(bits(scale), bits(want_scale)), "edge_scale"
    else:
        assert scale is None
    assert np.array_equal(bits(gx), bits(want_gx)), "grad_x"
    return out, scale, gx


# ---------------------------------------------------------------- 1 bitwise against the restatement
# every dim with R = 5, every R with dim 3 (element-wise route, 16 lanes) and 128 (16-byte pieces, 32 lanes)
CASES = [(d, 5) for d in (1, 3, 4, 33, 100, 128, 256)] + [(d, R) for R in (1, 2, 37) for d in (3, 128)]


@pytest.mark.parametrize("dim,R", CASES)
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_bitwise_power_law_block_with_chunked_hub(gpu_env, dim, R, aggr):
    from wholegraph_amd.torch.aggregation import chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(1000 * R + dim)
    n_dst, n_src = 300, 900
    row_ptr, col, et = typed_block(rng, R, n_dst, n_src)
    deg = np.diff(row_ptr)
    counts = np.bincount(col, minlength=n_src)
    assert counts[7] > 2 * C, "the hub must run into a third chunk"
    assert {0, 1, 70} <= set(deg.tolist()) and n_src > n_dst
    assert (counts[:n_dst] == 0).any() and (counts[n_dst:] == 0).any()
    if R >= 2:
        assert not (et == R - 1).any()
    if R >= 3:
        present = np.zeros((n_dst, R), bool)
        present[np.repeat(np.arange(n_dst), deg), et] = True
        assert (present.sum(1)[deg > 0] <= R - 2).all() and present.sum(1).max() >= 2
    if R >= 4:
        first = row_ptr[1]
        assert len(set(et[first:first + 70].tolist())) >= 2, "types are interleaved within a target"
    x = rng.standard_normal((n_src, dim)).astype(F32)
    g = rng.standard_normal((n_dst, (R + 1) * dim)).astype(F32)
    g[5, R * dim:] = -0.0
    check_bitwise(x, row_ptr, col, et, R, g, aggr)


@pytest.mark.parametrize("dim", [5, 8])
def test_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, dim):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third;
    three relations, one edge in 50 with a type out of range"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    C, R = chunk_edges(), 3
    rng = np.random.default_rng(900 + dim)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    et = rng.integers(0, R, len(col)).astype(np.int32)
    et[rng.random(len(col)) < 0.02] = R
    x = rng.standard_normal((LR.N_SRC, dim)).astype(F32)
    g = rng.standard_normal((LR.N_DST, (R + 1) * dim)).astype(F32)
    for aggr in ("mean", "sum"):
        check_bitwise(x, row_ptr, col, et, R, g, aggr)


@pytest.mark.parametrize("dim", [3, 128])
def test_bitwise_strided_misaligned_x_and_int64_indices(gpu_env, dim):
    """a view with a row stride of its own that starts 1 float (4 bytes) into a row of dim + 9: the element-wise route;
    row_ptr, col_ind and edge_type as int64 tensors"""
    rng = np.random.default_rng(11)
    R, n_dst, n_src = 4, 97, 400
    row_ptr, col, et = typed_block(rng, R, n_dst, n_src, hub2=350)
    wide = rng.standard_normal((n_src, dim + 9)).astype(F32)
    xv = dev(wide)[:, 1:1 + dim]
    assert xv.stride(0) == dim + 9 and not xv.is_contiguous() and xv.data_ptr() % 16 == 4
    g = rng.standard_normal((n_dst, (R + 1) * dim)).astype(F32)
    for aggr in ("mean", "sum"):
        check_bitwise(wide[:, 1:1 + dim].copy(), row_ptr, col, et, R, g, aggr, x_dev=xv, wide_index=True)


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_empty_blocks(gpu_env, aggr):
    """E = 0: every slot is +0.0, the self copy is there, grad_x = (the self term for s < n_dst, +0.0 after). n_dst = 0: out
    has no row and grad_x is +0.0"""
    rng = np.random.default_rng(2)
    R, n_src, dim = 3, 50, 12
    x = rng.standard_normal((n_src, dim)).astype(F32)
    none_i = np.zeros(0, np.int32)
    g = rng.standard_normal((5, (R + 1) * dim)).astype(F32)
    out, scale, gx = check_bitwise(x, np.zeros(6, np.int32), none_i, none_i, R, g, aggr)
    assert not bits(out[:, :R * dim]).any() and np.array_equal(bits(out[:, R * dim:]), bits(x[:5]))
    assert np.array_equal(bits(gx[:5]), bits(g[:, R * dim:])) and not bits(gx[5:]).any()
    out, scale, gx = check_bitwise(x, np.zeros(1, np.int32), none_i, none_i, R, np.zeros((0, (R + 1) * dim), F32), aggr)
    assert out.shape == (0, (R + 1) * dim) and gx.shape == (n_src, dim) and not bits(gx).any()


# ---------------------------------------------------------------- 2 identities with the shipped op
@pytest.mark.parametrize("dim", [3, 128])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_one_relation_is_agg_concat(gpu_env, dim, aggr):
    from wholegraph_amd.torch.aggregation import agg_concat
    rng = np.random.default_rng(41)
    n_dst, n_src = 300, 900
    row_ptr, col, et = typed_block(rng, 1, n_dst, n_src)
    x = rng.standard_normal((n_src, dim)).astype(F32)
    g = rng.standard_normal((n_dst, 2 * dim)).astype(F32)
    out, _, gx = run_op(x, row_ptr, col, et, 1, g, aggr)
    xd = dev(x).requires_grad_(True)
    plain = agg_concat(xd, dev(row_ptr), dev(col), aggr)
    plain.backward(dev(g))
    assert np.array_equal(bits(out), bits(plain)) and np.array_equal(bits(gx), bits(xd.grad))


@pytest.mark.parametrize("dim", [3, 128])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_slot_r_is_agg_concat_on_the_sub_block_of_relation_r(gpu_env, dim, aggr):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.rel_aggregation import agg_concat_rel
    rng = np.random.default_rng(43)
    R, n_dst, n_src = 4, 200, 700
    row_ptr, col, _ = typed_block(rng, R, n_dst, n_src, hub2=650)
    et = rng.integers(0, R, len(col)).astype(np.int32)          # every relation present
    dst = np.repeat(np.arange(n_dst), np.diff(row_ptr))
    x = dev(rng.standard_normal((n_src, dim)).astype(F32))
    out = agg_concat_rel(x, dev(row_ptr), dev(col), dev(et), R, aggr)
    assert out.grad_fn is None and not out.requires_grad        # x asks for no gradient: no backward is queued
    for r in range(R):
        keep = et == r                                           # (boolean selection keeps the relative edge order)
        sub_ptr = np.zeros(n_dst + 1, np.int32)
        np.cumsum(np.bincount(dst[keep], minlength=n_dst), out=sub_ptr[1:])
        sub = agg_concat(x, dev(sub_ptr), dev(col[keep]), aggr)
        assert torch.equal(out[:, r * dim:(r + 1) * dim].view(torch.int32), sub[:, :dim].view(torch.int32)), r
    assert torch.equal(out[:, R * dim:].view(torch.int32), x[:n_dst].view(torch.int32))


# ---------------------------------------------------------------- 3 types out of range
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("wide_index", [False, True])
def test_out_of_range_types_contribute_nothing(gpu_env, aggr, wide_index):
    """-1, R and a large value sprinkled in: forward and edge_scale are those of the block with these edges deleted (and
    their edge_scale is +0.0); grad_x is the restatement's, and — no source here has more than C edges — also that of the
    block with the edges deleted"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(77)
    R, n_dst, n_src, dim = 5, 120, 400, 36
    row_ptr, col, et = typed_block(rng, R, n_dst, n_src, hub_share=0.02, hub2=350)
    assert np.bincount(col).max() <= chunk_edges() and np.diff(row_ptr).max() == 70
    et = rng.integers(0, R, len(col)).astype(np.int64 if wide_index else np.int32)
    big = [2 ** 31 - 1, -2 ** 31] + ([2 ** 40, 2 ** 32, 2 ** 32 + 1, -2 ** 40] if wide_index else [])
    junk = np.array([-1, R, R + 1] + big, et.dtype)
    bad = rng.random(len(col)) < 0.25
    et[bad] = junk[rng.integers(0, len(junk), int(bad.sum()))]
    et[row_ptr[4]:row_ptr[5]] = -1                                # a target all of whose edges are out of range
    bad = (et < 0) | (et >= R)
    col = col.copy()
    col[bad & (rng.random(len(col)) < 0.5)] = n_src - 1            # (their sources are never read, whatever they are)
    x = rng.standard_normal((n_src, dim)).astype(F32)
    g = rng.standard_normal((n_dst, (R + 1) * dim)).astype(F32)
    out, scale, gx = check_bitwise(x, row_ptr, col, et, R, g, aggr, wide_index=wide_index)
    # ... the same block with those edges deleted
    dst = np.repeat(np.arange(n_dst), np.diff(row_ptr))
    keep = ~bad
    sub_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(np.bincount(dst[keep], minlength=n_dst), out=sub_ptr[1:])
    want_out, want_scale = ref_forward(sub_ptr, col[keep], et[keep], R, x, aggr)
    want_gx = ref_grad_x(sub_ptr, col[keep], et[keep], R, want_scale, g, n_src, chunk_edges(), aggr)
    assert np.array_equal(bits(out), bits(want_out)) and np.array_equal(bits(gx), bits(want_gx))
    assert not bits(out[4, :R * dim]).any()
    if aggr == "mean":
        assert np.array_equal(bits(scale)[keep], bits(want_scale)) and not bits(scale)[bad].any()


@pytest.mark.parametrize("aggr", ["mean", "sum"])
def test_out_of_range_types_keep_their_place_in_the_chunks(gpu_env, aggr):
    """source 20: C + 40 edges, the first C + 8 of them out of range (its first chunk adds nothing, the second does);
    source 21: C + 5 edges, all out of range (no term at all: +0.0); source 1, a target: the same, so its self term alone.
    Every target here has more edges than a wave has lanes"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(5)
    R, n_dst, n_src, dim = 3, 16, 30, 8
    cols = [20] * (C + 40) + [21] * (C + 5) + [1] * (C + 5) + [22] * 40
    types_ = [-1] * (C + 8) + list(rng.integers(0, R, 32)) + [R] * (C + 5) + [7] * (C + 5) + list(rng.integers(0, R, 40))
    col, et = np.array(cols, np.int32), np.array(types_, np.int32)
    perm = np.concatenate([np.arange(C + 40), C + 40 + rng.permutation(len(col) - C - 40)])   # (source 20's order is kept)
    col, et = col[perm], et[perm]
    deg = np.full(n_dst, len(col) // n_dst, np.int64)
    deg[:len(col) % n_dst] += 1
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    x = rng.standard_normal((n_src, dim)).astype(F32)
    g = rng.standard_normal((n_dst, (R + 1) * dim)).astype(F32)
    out, scale, gx = check_bitwise(x, row_ptr, col, et, R, g, aggr)
    assert bits(gx[20]).any() and not bits(gx[21]).any()
    assert np.array_equal(bits(gx[1]), bits(g[1, R * dim:]))


# ---------------------------------------------------------------- 4 hand-derived bits, determinism
def test_products_round_before_the_add(gpu_env):
    """MEAN backward: source 3 is read by target 0 (its only edge of relation 0: scale 1, gradient -p) and by target 1 (one
    of its three edges of relation 0: scale s = fl(1/3), gradient 3). s * 3 is not a float; p = fl(s * 3). -p + fl(s * 3) is
    +0.0; a fused multiply-add would leave the rounding error of the product."""
    s = F32(1.0) / F32(3.0)
    p = F32(s * F32(3.0))
    assert float(s) * 3.0 != float(p)
    row_ptr = np.array([0, 1, 4], np.int32)
    col = np.array([3, 3, 2, 2], np.int32)
    et = np.zeros(4, np.int32)
    x = np.zeros((4, 1), F32)
    g = np.array([[-p, 0.0], [3.0, 0.0]], F32)
    out, scale, gx = check_bitwise(x, row_ptr, col, et, 1, g, "mean")
    assert bits(scale).tolist() == [0x3F800000] + [int(bits(np.array([s]))[0])] * 3
    assert bits(gx)[3, 0] == 0x00000000


@pytest.mark.parametrize("deg", [2, 70])
def test_signed_zeros(gpu_env, deg):
    """a slot without an edge is +0.0; a sum of -0.0 terms starts from its first term and stays -0.0, for SUM and (times
    1 / n) for MEAN — with few edges and with more than a wave of them"""
    R = 3
    row_ptr = np.array([0, deg, deg], np.int32)
    col = np.array([2, 3] * (deg // 2), np.int32)
    et = np.array([0, 2] * (deg // 2), np.int32)           # relation 1 is absent
    x = np.array([[1.0, 1.0], [1.0, 1.0], [-0.0, 0.0], [-0.0, -0.0]], F32)
    g = np.zeros((2, (R + 1) * 2), F32)
    for aggr in ("sum", "mean"):
        out, _, gx = check_bitwise(x, row_ptr, col, et, R, g, aggr)
        assert bits(out)[0].tolist() == [NEG0, 0, 0, 0, NEG0, NEG0, 0x3F800000, 0x3F800000]
        assert bits(out)[1, :6].tolist() == [0] * 6            # no edge at all: +0.0 in every slot


def test_two_calls_give_identical_bits(gpu_env):
    import torch
    rng = np.random.default_rng(9)
    R, dim = 5, 64
    row_ptr, col, et = typed_block(rng, R)
    x = rng.standard_normal((900, dim)).astype(F32)
    g = rng.standard_normal((300, (R + 1) * dim)).astype(F32)
    runs = [run_op(x, row_ptr, col, et, R, g, "mean") for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------- 5 the layer
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("num_bases", [None, 2])
def test_layer_is_linear_of_the_op(gpu_env, aggr, root_weight, bias, num_bases):
    import torch
    from wholegraph_amd.torch.cugraphops import RGCNConv
    from wholegraph_amd.torch.rel_aggregation import agg_concat_rel
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    R, n_dst, n_src, cin, cout = 4, 150, 600, 48, 24
    row_ptr, col, _ = typed_block(rng, R, n_dst, n_src, hub2=550)
    et = rng.integers(0, R, len(col)).astype(np.int32)
    rp, ci, ty = dev(row_ptr), dev(col), dev(et)
    layer = RGCNConv(cin, cout, R, num_bases=num_bases, aggr=aggr, root_weight=root_weight, bias=bias).cuda()
    if bias:
        torch.nn.init.normal_(layer.bias)
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, 70, ty)
    assert out.shape == (n_dst, cout)
    agg = agg_concat_rel(x, rp, ci, ty, R, aggr)
    W = layer.weight if num_bases is None else (layer.comp @ layer.weight.view(num_bases, -1)).view(R, cin, cout)
    want = agg[:, :R * cin] @ W.view(R * cin, cout)
    if root_weight:
        want = want + agg[:, R * cin:] @ layer.root
    if bias:
        want = want + layer.bias
    assert torch.equal(out, want)
    out.square().sum().backward()
    params = dict(layer.named_parameters())
    assert sorted(params) == sorted(["weight"] + (["comp"] if num_bases else []) + (["root"] if root_weight else []) +
                                    (["bias"] if bias else []))
    for name, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0


def test_layer_under_autocast_and_16_bit_rows_outside_it(gpu_env):
    import torch
    from wholegraph_amd.torch.cugraphops import RGCNConv
    from wholegraph_amd.torch.rel_aggregation import agg_concat_rel
    torch.manual_seed(0)
    rng = np.random.default_rng(22)
    R, n_dst, n_src, cin = 3, 120, 500, 32
    row_ptr, col, _ = typed_block(rng, R, n_dst, n_src, hub2=450)
    et = rng.integers(0, R, len(col)).astype(np.int32)
    rp, ci, ty = dev(row_ptr), dev(col), dev(et)
    x16 = dev(rng.standard_normal((n_src, cin)).astype(F32)).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = agg_concat_rel(x16, rp, ci, ty, R, "mean")
    assert got.dtype == torch.float32
    assert torch.equal(got, agg_concat_rel(x16.float(), rp, ci, ty, R, "mean"))
    layer = RGCNConv(cin, 8, R, num_bases=2).cuda()
    x = x16.float().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, rp, ci, 70, ty)
    assert out.shape == (n_dst, 8) and torch.isfinite(out).all()
    out.float().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    for bad in (x16, x16.half()):
        with pytest.raises(TypeError, match="float32"):
            agg_concat_rel(bad, rp, ci, ty, R, "mean")


# ---------------------------------------------------------------- 6 end to end
def _wm_array(comm, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


N_NODES, N_REL, FEAT = 500, 3, 16


def _typed_graph(comm):
    import wholegraph_amd.torch as wgth
    rng = np.random.default_rng(31)
    deg = rng.integers(1, 13, N_NODES)
    row_ptr = np.zeros(N_NODES + 1, np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = np.concatenate([rng.choice(N_NODES, int(k), replace=False) for k in deg]).astype(np.int64)
    etype = rng.integers(0, N_REL, len(col)).astype(np.int32)
    ts = [_wm_array(comm, a) for a in (row_ptr, col, etype)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("etype", ts[2])
    return g, ts, etype


def _rgcn_model(comm, g, feats):
    import torch
    import wholegraph_amd.torch as wgth
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [N_NODES, FEAT])
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(torch.from_numpy(feats).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    torch.cuda.synchronize()
    wgth.set_framework("cugraph")
    args = types.SimpleNamespace(model="rgcn", hiddensize=32, layernum=2, classnum=4, dropout=0.1, neighbors="5,5",
                                 inferencesample="5,5", num_relations=N_REL, edge_type_name="etype", num_bases=2)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    assert [type(l).__name__ for l in model.gnn_layers] == ["RGCNConv", "RGCNConv"] and not model.add_self_loop
    assert all(l.num_relations == N_REL and l.num_bases == 2 for l in model.gnn_layers)
    return model, emb, wm_opt


def _two_steps(comm, g, feats, labels):
    """a fresh model, two training steps -> (the logits of both steps, the embedding table after them: the gradients that
    reached it, applied by the WholeMemory SGD optimizer)"""
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    torch.manual_seed(1)
    random.seed(1)   # (the sampler draws its per-hop seeds from `random`)
    rng = np.random.default_rng(2)
    model, emb, wm_opt = _rgcn_model(comm, g, feats)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    model.train()
    logits_seen = []
    for step in range(2):
        ids = torch.from_numpy(rng.choice(N_NODES, 64, replace=False).astype(np.int64)).cuda()
        logits = model(ids)
        assert logits.shape == (64, 4) and torch.isfinite(logits).all()
        loss = Fn.cross_entropy(logits, labels[ids])
        opt.zero_grad()
        loss.backward()
        opt.step()
        wm_opt.step(0.05)
        logits_seen.append(logits.detach().clone())
    torch.cuda.synchronize()
    table = emb.get_embedding_tensor().get_local_tensor()[0].clone()
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    return logits_seen, table


def test_rgcn_model_end_to_end_is_reproducible_and_gets_the_sampled_edge_types(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    g, ts, etype = _typed_graph(gpu_env)
    rng = np.random.default_rng(9)
    feats = rng.standard_normal((N_NODES, FEAT)).astype(F32)
    labels = dev(rng.integers(0, 4, N_NODES).astype(np.int64))
    la, ta = _two_steps(gpu_env, g, feats, labels)
    lb, tb = _two_steps(gpu_env, g, feats, labels)
    for a, b in zip(la, lb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert bool((ta != dev(feats)).any()), "no gradient reached the WholeMemory embedding"
    # the types each layer receives are the attribute at the graph edges the sampler drew
    model, emb, wm_opt = _rgcn_model(gpu_env, g, feats)
    seen = []
    for layer in model.gnn_layers:
        layer.register_forward_pre_hook(lambda mod, a: seen.append((a[1], a[2], a[4])))
    ids = torch.arange(0, N_NODES, 7, device="cuda")
    model.train()
    random.seed(5)
    model(ids)
    random.seed(5)
    _, _, rps, cis, attrs = g.multilayer_sample_with_edge_attributes(ids, [5, 5], ["__edge_id__"])
    assert len(seen) == 2
    for i, (rp, ci, ty) in enumerate(seen):
        assert torch.equal(rp, rps[i]) and torch.equal(ci, cis[i])
        assert ty.shape == ci.shape and ty.dtype == torch.int32
        assert np.array_equal(ty.cpu().numpy(), etype[attrs[i]["__edge_id__"].cpu().numpy()])
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    for t in ts:
        wgth.destroy_wholememory_tensor(t)
