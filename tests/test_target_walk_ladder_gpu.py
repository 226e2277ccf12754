"""Every block op, forward and backward, on a degree ladder: target d has exactly d edges and source s a run of exactly s
sorted positions, d and s = 0 .. 130.

The per-target walk and the batch walk of csrc/kernels/agg_common.cuh (for_target_pieces, for_edge_batches) take LANES
positions at a time, LANES = 16 / 32 / 64, and a batch of rows at a time within those. What can go wrong there goes wrong at
a boundary: a range of exactly LANES positions, of one fewer, of one more, a ragged last batch of one row. The block of
tests/_capped_block.py has the degrees 0, 1, 8, 9, 17 and 65 and random ones in 25 .. 46; the ladder has every range length
from 0 to 2 * 64 + 2 on the targets' side and, because col is a permutation of repeat(arange(131), arange(131)), on the
sources' side as well, at every lane width. 8515 edges; the grid cap is unset.

Every output is compared with the references of the op's own test file, imported from there as
tests/test_block_ops_capped_grid_gpu.py imports them: the numpy restatement of the stated order, bit for bit; attention alpha
within the bound of its float64 softmax, everything downstream restated from the op's own alpha.

Row widths: 8, 128, 320 and 3 (16-bit rows: 8, 256, 640 and 3) are 16, 32 and 64 lanes on 16-byte pieces, the last with a
second column pass, and the element-wise instantiation. (H, F) of the attention ops: (2, 4), (2, 64) and (3, 128) likewise,
(2, 3) element-wise."""
import functools

import numpy as np
import pytest

import test_block_ops_capped_grid_gpu as CG

pytestmark = pytest.mark.gpu

F32 = np.float32
N_DST, N_SRC = 131, 140
N_EDGES = 130 * 131 // 2
WIDTHS = [8, 128, 320, 3]
WIDTHS16 = [8, 256, 640, 3]
HEADS = [(2, 4), (2, 64), (3, 128), (2, 3)]
AGGRS = ["mean", "sum"]
dev, np_of, same = CG.dev, CG.np_of, CG.same


@functools.lru_cache(maxsize=None)
def ladder():
    """(row_ptr [N_DST + 1] int32, col [N_EDGES] int32), read-only"""
    deg = np.arange(N_DST)
    row_ptr = np.zeros(N_DST + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = np.random.default_rng(131).permutation(np.repeat(np.arange(N_DST), deg)).astype(np.int32)
    for a in (row_ptr, col):
        a.setflags(write=False)
    return row_ptr, col


@pytest.fixture
def block(gpu_env, knobs):
    """(C, row_ptr, col) with the grid cap unset; the device tensors behind a case's outputs are dropped after it"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    knobs.unset(CG.KNOB)
    yield (chunk_edges(),) + ladder()
    CG._ALIVE.clear()


def test_the_ladder_has_every_range_length_on_both_walks():
    row_ptr, col = ladder()
    assert len(col) == N_EDGES == 8515 and row_ptr[-1] == N_EDGES
    assert np.array_equal(np.diff(row_ptr), np.arange(N_DST))                                  # target d: d edges
    assert np.array_equal(np.bincount(col, minlength=N_SRC), np.r_[np.arange(N_DST), [0] * (N_SRC - N_DST)])   # source s: s
    assert N_DST - 1 >= 2 * 64 + 2
    dst = np.repeat(np.arange(N_DST), np.diff(row_ptr))
    assert (col != dst).any() and len(np.unique(col[row_ptr[130]:row_ptr[131]])) > 1          # (a permutation, not the identity)


# ---------------------------------------------------------------- the agg_concat family
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat(block, dim, aggr):
    import test_sage_agg_gpu as T
    from wholegraph_amd.torch.aggregation import agg_concat
    C_, row_ptr, col = block
    rng = np.random.default_rng(100 + dim)
    x_np = rng.standard_normal((N_SRC, dim)).astype(F32)
    g_np = rng.standard_normal((N_DST, 2 * dim)).astype(F32)
    x = dev(x_np).requires_grad_(True)
    out = agg_concat(x, dev(row_ptr), dev(col), aggr)
    out.backward(dev(g_np))
    same(np_of(out), T.ref_forward(row_ptr, col, x_np, aggr), "out")
    same(np_of(x.grad), T.ref_backward(row_ptr, col, g_np, N_SRC, aggr, C_), "grad_x")


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS16)
@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_agg_concat_16_bit(block, name, dim, aggr):
    import test_sage_agg_half_gpu as T
    from wholegraph_amd.torch.aggregation import agg_concat
    C_, row_ptr, col = block
    rng = np.random.default_rng(200 + dim)
    xb, x32 = T.random_rows(rng, (N_SRC, dim), name)
    gb, g32 = T.random_rows(rng, (N_DST, 2 * dim), name)
    x = T.dev16(xb, name).requires_grad_(True)
    out = agg_concat(x, dev(row_ptr), dev(col), aggr)
    out.backward(T.dev16(gb, name))
    assert out.dtype == T.tdtype(name) and x.grad.dtype == T.tdtype(name)
    same(np_of(out), T.round_bits(T.ref_forward(row_ptr, col, x32, aggr), name), "out")
    same(np_of(x.grad), T.round_bits(T.ref_backward(row_ptr, col, g32, N_SRC, aggr, C_), name), "grad_x")


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat_weighted(block, dim, aggr):
    import test_weighted_agg_gpu as T
    import wholegraph_amd.torch.weighted_aggregation as wa
    C_, row_ptr, col = block
    rng = np.random.default_rng(300 + dim)
    x_np = rng.standard_normal((N_SRC, dim)).astype(F32)
    w_np = rng.standard_normal(N_EDGES).astype(F32)
    g_np = rng.standard_normal((N_DST, 2 * dim)).astype(F32)
    record = list(wa.backward_requests)   # (a bounded record that test_weighted_agg_gpu.py counts on: left as it was found)
    try:
        out, gx, gw = T.run_op(x_np, np.array(row_ptr), np.array(col), w_np, g_np, aggr)
    finally:
        wa.backward_requests[:] = record
    want_out, want_gx, want_gw = T.ref_all(row_ptr, col, w_np, x_np, g_np, aggr, C_)
    same(np_of(out), want_out, "out")
    same(np_of(gx), want_gx, "grad_x")
    same(np_of(gw), want_gw, "grad_w")


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat_rel(block, dim, aggr):
    import test_rel_agg_gpu as T
    C_, row_ptr, col = block
    R = 3
    rng = np.random.default_rng(400 + dim)
    et = rng.integers(0, R, N_EDGES).astype(np.int32)
    et[rng.random(N_EDGES) < 0.02] = R            # types out of range: they keep their place and add nothing
    et[rng.random(N_EDGES) < 0.02] = -1
    x_np = rng.standard_normal((N_SRC, dim)).astype(F32)
    g_np = rng.standard_normal((N_DST, (R + 1) * dim)).astype(F32)
    want_out, want_scale = T.ref_forward(row_ptr, col, et, R, x_np, aggr)
    out, scale, gx = T.run_op(x_np, np.array(row_ptr), np.array(col), et, R, g_np, aggr)
    same(np_of(out), want_out, "out")
    assert (scale is not None) == (aggr == "mean")
    if scale is not None:
        same(np_of(scale), want_scale, "edge_scale")
    same(np_of(gx), T.ref_grad_x(row_ptr, col, et, R, want_scale, g_np, N_SRC, C_, aggr), "grad_x")


@pytest.mark.parametrize("dtype,dim", [("float32", d) for d in WIDTHS] + [("bfloat16", 256), ("float16", 3)])
def test_gather_agg_concat(gpu_env, block, dtype, dim):
    import torch
    import test_gather_agg_gpu as T
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    C_, row_ptr, col = block
    n_rows = 5003
    rng = np.random.default_rng(500 + dim)
    values = T.table_values(rng, n_rows, dim, getattr(torch, dtype))
    ids = rng.integers(0, n_rows, N_SRC)
    ids[:3] = [0, n_rows - 1, 0]
    x_np = values.float().numpy()[ids]
    emb = T.make_embedding(gpu_env, "chunked", "cuda", getattr(torch, dtype), values)
    try:
        for aggr in AGGRS:
            before = gather_aggregation.calls()
            out = wgth.gather_agg_concat(emb, dev(ids), dev(row_ptr), dev(col), aggr)
            assert gather_aggregation.calls() == before + 1, "the fused kernel did not run"
            same(np_of(out), T.ref_forward(row_ptr, col, x_np, aggr), aggr + ": out")
    finally:
        wgth.destroy_embedding(emb)


@pytest.mark.parametrize("dim", WIDTHS)
def test_gather_agg_concat_quantized(gpu_env, block, dim):
    import test_qagg_gpu as T
    import wholegraph_amd.torch as wgth
    from test_qrows_gpu import destroy, make_table, raw_of, reference
    from wholegraph_amd.torch import gather_aggregation
    C_, row_ptr, col = block
    n_rows = T.N_ROWS
    x, _, _ = reference(n_rows, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=4)
    try:
        ids = np.random.default_rng(600 + dim).integers(0, n_rows, N_SRC)
        ids[:3] = [0, n_rows - 1, 0]
        raw = raw_of(t).cpu().numpy().view(np.uint8)   # the table's bytes, read by the row gather (no block op)
        for aggr in AGGRS:
            before = gather_aggregation.quantized_calls()
            out = wgth.gather_agg_concat(t, dev(ids), dev(row_ptr), dev(col), aggr)
            assert gather_aggregation.quantized_calls() == before + 1, "the fused kernel did not run"
            same(np_of(out), T.numpy_forward(raw, dim, ids, row_ptr, col, aggr), aggr + ": out")
    finally:
        destroy(t)


@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat_pna(block, dim):
    import test_pna_gpu as T
    C_, row_ptr, col = block
    names = T.ORDER
    rng = np.random.default_rng(700 + dim)
    x_np = rng.standard_normal((N_SRC, dim)).astype(F32)
    x_np[:, 0] = 2.0                                   # ties in min / max, a variance of exactly zero
    g_np = rng.standard_normal((N_DST, (len(names) + 1) * dim)).astype(F32)
    want_out, want_saved = T.ref_forward(row_ptr, col, x_np, names)
    out, saved, gx = T.run_op(x_np, np.array(row_ptr), np.array(col), names, g_np)
    same(np_of(out), want_out, "out")
    assert len(saved) == 4 and all(s is not None for s in saved)
    for n, s, w in zip(("arg_min", "arg_max", "std_mean", "std_coef"), saved, want_saved):
        same(np_of(s), w, n)
    same(np_of(gx), T.ref_backward(row_ptr, col, x_np, names, want_saved, g_np, C_), "grad_x")


@pytest.mark.parametrize("F", WIDTHS + [64])
def test_edge_dot(block, F):
    """8 and 64: the lane-split tree at 16 lanes; 128: at 32 lanes; 320 and 3: the element-wise forward"""
    import test_edge_dot_gpu as T
    C_, row_ptr, col = block
    rng = np.random.default_rng(800 + F)
    xs_np, xd_np = T.rows(rng, N_SRC, N_DST, F)
    g_np = rng.standard_normal(N_EDGES).astype(F32)
    score, grads = T.run_op(dev(xs_np), dev(xd_np), row_ptr, col, g_np)
    want_s, want_gs, want_gd = T.ref_all(row_ptr, col, xs_np, xd_np, g_np, C_)
    same(np_of(score), want_s, "score")
    same(np_of(grads[0]), want_gs, "grad_src")
    same(np_of(grads[1]), want_gd, "grad_dst")


# ---------------------------------------------------------------- the attention ops
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F", HEADS)
def test_mha_gat_n2n(block, H, F, concat):
    import test_gat_gpu as T
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    C_, row_ptr, col = block
    rng = np.random.default_rng(900 + 10 * H + F + concat)
    h_np, att_np = T.inputs(rng, N_SRC, H, F)
    G_np = rng.standard_normal((N_DST, H * F if concat else F)).astype(F32)
    ref, bound = T.ref_alpha64(row_ptr, col, h_np, att_np, H, 0.2)
    h, att = dev(h_np).requires_grad_(True), dev(att_np).requires_grad_(True)
    out, alpha = mha_gat_n2n(h, att, dev(row_ptr), dev(col), H, 0.2, concat, return_alpha=True)
    out.backward(dev(G_np))
    al = np_of(alpha)
    CG.check_alpha(al, ref, bound, "mha_gat_n2n")
    gh, ga = T.ref_backward(row_ptr, col, h_np, att_np, al, G_np, H, 0.2, concat, C_, node_chunk())
    same(np_of(out), T.ref_out(row_ptr, col, h_np, al, H, concat), "out")
    same(np_of(h.grad), gh, "grad_h")
    same(np_of(att.grad), ga, "grad_att")


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F", HEADS)
def test_mha_gat_n2n_with_edge_features(block, H, F, concat):
    import test_gat_edge_gpu as T
    from test_gat_gpu import inputs, ref_out
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    C_, row_ptr, col = block
    rng = np.random.default_rng(1000 + 10 * H + F + concat)
    h_np, att = inputs(rng, N_SRC, H, F)
    att_np = np.concatenate([att, (0.5 * rng.standard_normal(H * F) / np.sqrt(F)).astype(F32)])
    ef_np = rng.standard_normal((N_EDGES, H * F)).astype(F32)
    G_np = rng.standard_normal((N_DST, H * F if concat else F)).astype(F32)
    s_edge = T.ref_edge_scores(ef_np, att_np, H)
    ref, bound = T.ref_alpha64_edge(row_ptr, T.ref_z(row_ptr, col, h_np, att_np, s_edge, H), 0.2)
    out, alpha, es, gh, ga, gef = T.run_op(h_np, att_np, dev(ef_np), np.array(row_ptr), np.array(col), H, concat, G_np)
    same(np_of(es), s_edge, "edge_scores")
    al = np_of(alpha)
    CG.check_alpha(al, ref, bound, "edge GAT")
    want_gh, want_ga, want_gef, _ = T.ref_backward_edge(row_ptr, col, h_np, att_np, ef_np, al, G_np, H, 0.2, concat, C_,
                                                        node_chunk())
    same(np_of(out), ref_out(row_ptr, col, h_np, al, H, concat), "out")
    same(np_of(gh), want_gh, "grad_h")
    same(np_of(ga), want_ga, "grad_att")
    same(np_of(gef), want_gef, "grad_edge_feat")


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F", HEADS)
def test_mha_gat_v2_n2n(block, H, F, concat):
    import test_gatv2_gpu as T
    from test_gat_gpu import ref_out
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    C_, row_ptr, col = block
    slope = 0.2
    rng = np.random.default_rng(1100 + 10 * H + F + concat)
    hs_np, hd_np, att_np = T.inputs(rng, N_SRC, N_DST, H, F)
    G_np = rng.standard_normal((N_DST, H * F if concat else F)).astype(F32)
    l32, _, _ = T.ref_logits(row_ptr, col, hs_np, hd_np, att_np, H, slope)
    ref, bound = T.ref_alpha64(row_ptr, l32)
    out, alpha, grads = T.run_op(dev(hs_np), dev(hd_np), att_np, np.array(row_ptr), np.array(col), G_np, H, slope, concat)
    al = np_of(alpha)
    CG.check_alpha(al, ref, bound, "mha_gat_v2_n2n")
    ghs, ghd, ga = T.ref_backward(row_ptr, col, hs_np, hd_np, att_np, al, G_np, H, slope, concat, C_, node_chunk())
    same(np_of(out), ref_out(row_ptr, col, hs_np, al, H, concat), "out")
    same(np_of(grads[0]), ghs, "grad_h_src")
    same(np_of(grads[1]), ghd, "grad_h_dst")
    same(np_of(grads[2]), ga, "grad_att")


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F", HEADS)
def test_mha_simple_n2n(block, H, F, concat):
    import test_tconv_gpu as T
    from test_gat_gpu import ref_out
    from test_gatv2_gpu import ref_alpha64
    C_, row_ptr, col = block
    norm = True
    rng = np.random.default_rng(1200 + 10 * H + F + concat)
    k_np, q_np, v_np = T.inputs(rng, N_SRC, N_DST, H, F)
    G_np = rng.standard_normal((N_DST, H * F if concat else F)).astype(F32)
    ref, bound = ref_alpha64(row_ptr, T.ref_logits(row_ptr, col, k_np, q_np, H, norm))
    out, alpha, grads = T.run_op(dev(k_np), dev(q_np), dev(v_np), np.array(row_ptr), np.array(col), G_np, H, concat, norm)
    al = np_of(alpha)
    CG.check_alpha(al, ref, bound, "mha_simple_n2n")
    gk, gq, gv = T.ref_backward(row_ptr, col, k_np, q_np, v_np, al, G_np, H, concat, norm, C_)
    same(np_of(out), ref_out(row_ptr, col, v_np, al, H, concat), "out")
    same(np_of(grads[0]), gk, "grad_key")
    same(np_of(grads[1]), gq, "grad_query")
    same(np_of(grads[2]), gv, "grad_value")
