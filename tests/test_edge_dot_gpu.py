"""The edge dot product on the MI355X (wholegraph_amd/torch/edge_dot.py -> csrc/kernels/edot.hip).

Scores and both gradients are checked bit for bit against a numpy restatement of the order the header states
(include/wholememory/wholegraph_amd_ext.h, section 2p), built from the restatements the attention tests already hold
(tree_sum, seg_sum, per_source), and with assert_close_scaled against torch autograd through the composite
``(x_dst[dst] * x_src[col]).sum(-1)`` at the tolerances the attention tests take (rtol 1e-5 for the scores, 1e-4 for the
gradients). Then every launch under a capped grid, with the harness of tests/test_block_ops_capped_grid_gpu.py."""
import numpy as np
import pytest

import _capped_block as CB
import _long_runs as LR
import test_block_ops_capped_grid_gpu as CG
from test_gat_gpu import assert_close_scaled, edge_dst, seg_sum
from test_gatv2_gpu import hub_block, tree_sum
from test_sage_agg_gpu import bits, block, dev
from test_tconv_gpu import per_source

pytestmark = pytest.mark.gpu

F32 = np.float32
WIDTHS = [1, 3, 4, 8, 32, 100, 128, 256, 512]


# ---------------------------------------------------------------- the order, restated
def ref_all(row_ptr, col, xs, xd, g, chunk):
    """(score, grad_src, grad_dst) in the stated order"""
    col = np.asarray(col, np.int64)
    dst = edge_dst(row_ptr)
    n_dst = len(row_ptr) - 1
    score = tree_sum(xd[dst] * xs[col]) if len(col) else np.zeros(0, F32)
    gd = seg_sum(row_ptr, g[:, None] * xs[col]) if n_dst else np.zeros((0, xs.shape[1]), F32)
    gs = per_source(col, xs.shape[0], g[:, None] * xd[dst], chunk)
    return score.astype(F32), gs, gd


def composite(xs, xd, row_ptr, col):
    import torch
    n_dst = row_ptr.numel() - 1
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=xs.device), deg)
    return (xd.index_select(0, dst) * xs.index_select(0, col.long())).sum(-1)


def run_op(xs_t, xd_t, row_ptr, col, g_np, need=(True, True), index=np.int32):
    """(score, [grad_src, grad_dst]) of one forward + backward; a gradient is None where need is False"""
    from wholegraph_amd.torch.edge_dot import edge_dot_n2n
    xs, xd = (t.detach().requires_grad_(n) for t, n in zip((xs_t, xd_t), need))
    score = edge_dot_n2n(xs, xd, dev(np.asarray(row_ptr, index)), dev(np.asarray(col, index)))
    if any(need):
        score.backward(dev(g_np))
    return score.detach(), [xs.grad, xd.grad]


def check_all(xs_np, xd_np, row_ptr, col, rng, tensors=None, loose=True):
    from wholegraph_amd.torch.aggregation import chunk_edges
    n_dst = len(row_ptr) - 1
    g_np = rng.standard_normal(len(col)).astype(F32)
    xs_t, xd_t = (dev(xs_np), dev(xd_np)) if tensors is None else tensors
    score, grads = run_op(xs_t, xd_t, row_ptr, col, g_np)
    assert score.shape == (len(col),) and grads[0].shape == xs_np.shape and grads[1].shape == xd_np.shape
    want_s, want_gs, want_gd = ref_all(row_ptr, col, xs_np, xd_np[:n_dst], g_np, chunk_edges())
    assert np.array_equal(bits(score), want_s.view(np.uint32)), "score"
    assert np.array_equal(bits(grads[0]), want_gs.view(np.uint32)), "grad_src"
    assert np.array_equal(bits(grads[1])[:n_dst], want_gd.view(np.uint32)), "grad_dst"
    assert not grads[1][n_dst:].any()
    if loose and len(col):
        xs2, xd2 = (dev(a).requires_grad_(True) for a in (xs_np, xd_np))
        want = composite(xs2, xd2, dev(row_ptr), dev(col))
        assert_close_scaled(score, want.detach(), 1e-5)
        want.backward(dev(g_np))
        assert_close_scaled(grads[0], xs2.grad)
        assert_close_scaled(grads[1], xd2.grad)
    return score, grads, g_np


def rows(rng, n_src, n_dst, F):
    return rng.standard_normal((n_src, F)).astype(F32), rng.standard_normal((n_dst, F)).astype(F32)


# ---------------------------------------------------------------- 1 every width on every block
@pytest.mark.parametrize("F", WIDTHS)
def test_bitwise_on_random_and_hub_blocks(gpu_env, F):
    """element-wise at 16 (F = 1, 3) and 64 lanes (100 forward, 512), the lane-split tree at 16 (4, 8), 32 (128) and 64
    lanes (256), 16-byte pieces without a tree (100 backward) and F beyond the lane-split limit (512); a block with empty
    targets and unread sources, and the hub block: a source with 2 C + 3 edges, targets of degree 0, 1, 8, 9, 17 and 2 C"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(3000 + F)
    row_ptr, col = block(rng, 300, 500, 12)
    assert (np.diff(row_ptr) == 0).any() and (np.bincount(col, minlength=500) == 0).any()
    xs, xd = rows(rng, 500, 300, F)
    check_all(xs, xd, row_ptr, col, rng)
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    xs, xd = rows(rng, n_src, n_dst, F)
    check_all(xs, xd, row_ptr, col, rng)


@pytest.mark.parametrize("F", [5, 8])
def test_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, F):
    from wholegraph_amd.torch.aggregation import chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(3100 + F)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    xs, xd = rows(rng, LR.N_SRC, LR.N_DST, F)
    check_all(xs, xd, row_ptr, col, rng, loose=False)


@pytest.mark.parametrize("F", [3, 32, 100])
def test_target_of_degree_70_and_more_targets_than_sources(gpu_env, F):
    """degree 70: more than 8 full batches of 8 rows and a ragged tail; 16 lanes see it as 4 full trips and a ragged fifth.
    The targets have rows of their own, so there may be more of them than source rows"""
    rng = np.random.default_rng(3200 + F)
    n_dst, n_src = 90, 40
    deg = rng.integers(0, 6, n_dst)
    deg[3], deg[50] = 70, 64
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n_src, int(row_ptr[-1])).astype(np.int32)
    xs, xd = rows(rng, n_src, n_dst, F)
    check_all(xs, xd, row_ptr, col, rng)


def test_empty_blocks(gpu_env):
    rng = np.random.default_rng(3300)
    F, n_src = 8, 50
    for n_dst in (0, 6):   # n_dst = 0, then E = 0 with targets
        xs, xd = rows(rng, n_src, n_dst, F)
        score, grads, _ = check_all(xs, xd, np.zeros(n_dst + 1, np.int32), np.zeros(0, np.int32), rng)
        assert score.numel() == 0
        assert all(np.array_equal(bits(g), np.zeros(g.shape, np.uint32)) for g in grads)   # +0.0


def test_block_from_skipgram_block(gpu_env):
    """the block the model trains on, from hand-made walks: contexts made unique by hand, duplicates among the centres"""
    import torch
    from wholegraph_amd.torch.skipgram import centers_of, skipgram_block
    walks = torch.tensor([[5, 9, 5, 2, 7, 9], [3, -1, -1, -1, -1, -1], [-1, -1, -1, -1, -1, -1], [2, 7, 2, 7, -1, -1],
                          [11, 4, -1, -1, -1, -1]], dtype=torch.int64)
    centres = centers_of(walks)
    negatives = (centres[:, None] * 7 + torch.arange(3)[None, :]) % 13
    negatives[::4, 1] = -1
    center_ids, row_ptr, ctx_ids, labels = skipgram_block(walks, 2, negatives)
    uniq, col = np.unique(ctx_ids.numpy(), return_inverse=True)
    assert len(center_ids) > len(uniq)
    rng = np.random.default_rng(3400)
    table = rng.standard_normal((13, 32)).astype(F32)
    check_all(table[uniq], table[center_ids.numpy()], row_ptr.numpy(), col.astype(np.int32), rng)


# ---------------------------------------------------------------- 2 routes
def test_strided_and_misaligned_views_equal_the_aligned_copy(gpu_env):
    import torch
    rng = np.random.default_rng(3500)
    F, n_dst, n_src = 32, 97, 260
    row_ptr, col = block(rng, n_dst, n_src, 30)
    wide_s = rng.standard_normal((n_src, F + 8)).astype(F32)
    wide_d = rng.standard_normal((n_dst + 3, F + 12)).astype(F32)   # rows behind the targets
    g = rng.standard_normal(len(col)).astype(F32)
    want = run_op(dev(wide_s[:, 4:4 + F].copy()), dev(wide_d[:, 4:4 + F].copy()), row_ptr, col, g)   # the lane-split tree
    for off in (4, 1):   # a stride > F on 16-byte pieces; then one element off: the element-wise route
        views = tuple(dev(w)[:, off:off + F] for w in (wide_s, wide_d))
        assert all(not t.is_contiguous() and t.stride(0) > F for t in views)
        assert all((t.data_ptr() % 16 != 0) == (off == 1) for t in views)
        xs, xd = wide_s[:, off:off + F].copy(), wide_d[:, off:off + F].copy()
        score, grads, g2 = check_all(xs, xd, row_ptr, col, np.random.default_rng(3501), tensors=views, loose=False)
        assert grads[1].shape[0] == n_dst + 3
        got = run_op(views[0], views[1], row_ptr, col, g)
        aligned = want if off == 4 else run_op(dev(xs), dev(xd), row_ptr, col, g)
        for a, b in zip([got[0]] + got[1], [aligned[0]] + aligned[1]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_gradient_subsets_int64_indices_and_repeated_calls(gpu_env):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(3600)
    xs, xd = (dev(a) for a in rows(rng, n_src, n_dst, 32))
    g = rng.standard_normal(len(col)).astype(F32)
    full = run_op(xs, xd, row_ptr, col, g)
    for other in (run_op(xs, xd, row_ptr, col, g), run_op(xs, xd, row_ptr, col, g, index=np.int64)):
        for a, b in zip([full[0]] + full[1], [other[0]] + other[1]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for need in ((False, True), (True, False), (False, False)):
        score, grads = run_op(xs, xd, row_ptr, col, g, need)
        assert torch.equal(score.view(torch.int32), full[0].view(torch.int32))
        assert [t is not None for t in grads] == list(need)
        for got, want in zip(grads, full[1]):
            assert got is None or torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_the_same_tensor_on_both_sides(gpu_env):
    """x_src is x_dst: autograd adds the two gradients, each the op's own bits"""
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    from wholegraph_amd.torch.edge_dot import edge_dot_n2n
    rng = np.random.default_rng(3700)
    n = 200
    row_ptr, col = block(rng, n, n, 12)
    x_np = rng.standard_normal((n, 16)).astype(F32)
    g_np = rng.standard_normal(len(col)).astype(F32)
    x = dev(x_np).requires_grad_(True)
    score = edge_dot_n2n(x, x, dev(row_ptr), dev(col))
    score.backward(dev(g_np))
    want_s, want_gs, want_gd = ref_all(row_ptr, col, x_np, x_np, g_np, chunk_edges())
    assert np.array_equal(bits(score), want_s.view(np.uint32))
    both = {(want_gs + want_gd).tobytes(), (want_gd + want_gs).tobytes()}   # (one fp32 add: commutative)
    assert x.grad.cpu().numpy().tobytes() in both


def test_16_bit_rows_under_autocast_and_outside_it(gpu_env):
    import torch
    from wholegraph_amd.torch.edge_dot import edge_dot_n2n
    rng = np.random.default_rng(3800)
    row_ptr, col = block(rng, 60, 200, 9)
    rp, ci = dev(row_ptr), dev(col)
    xs, xd = (dev(a).bfloat16() for a in rows(rng, 200, 60, 16))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        score = edge_dot_n2n(xs, xd, rp, ci)
    assert score.dtype == torch.float32
    assert torch.equal(score.view(torch.int32), edge_dot_n2n(xs.float(), xd.float(), rp, ci).view(torch.int32))
    for args in ((xs, xd.float()), (xs.float(), xd)):
        with pytest.raises(TypeError, match="float32"):
            edge_dot_n2n(*args, rp, ci)


# ---------------------------------------------------------------- 3 under a capped grid
# launch sites: edot_fwd_kernel and edot_bwd_dst_kernel (301 targets), agg_bwd_prep_kernel (one thread per edge),
# edot_bwd_chunk_kernel (21 tiles: 2 workgroups of 16 groups and more of fewer), edot_bwd_fold_kernel (1103 sources). Each
# wants more than one workgroup at every width: full = 0.
@pytest.mark.parametrize("F", CG.WIDTHS + [64])
def test_under_a_capped_grid(gpu_env, knobs, F):
    """8 and 64: the lane-split tree and the 16-byte backward at 16 lanes (2 pieces; 16 pieces, every lane of a group in the
    tree); 128: both at 32 lanes; 320: the element-wise forward at 64 lanes with lanes that take a second edge, the 16-byte
    backward at 64 lanes with a second column pass of 48 inactive lanes; 3 and 33: element-wise at 16 and 64 lanes"""
    C_, row_ptr, col = CG.the_block()
    rng = np.random.default_rng(3900 + F)
    xs_np, xd_np = rows(rng, CB.N_SRC, CB.N_DST, F)
    g_np = rng.standard_normal(len(col)).astype(F32)
    want_s, want_gs, want_gd = ref_all(row_ptr, col, xs_np, xd_np, g_np, C_)

    def run(other):
        from wholegraph_amd.torch.edge_dot import edge_dot_n2n
        xs = CG.dev(CG.alt(xs_np, other)).requires_grad_(True)
        xd = CG.dev(CG.alt(xd_np, other)).requires_grad_(True)
        score = edge_dot_n2n(xs, xd, CG.dev(row_ptr), CG.dev(col))
        score.backward(CG.dev(CG.alt(g_np, other)))
        return {"score": CG.np_of(score), "grad_src": CG.np_of(xs.grad), "grad_dst": CG.np_of(xd.grad)}

    def check(o, label):
        CG.same(o["score"], want_s, label + ": score")
        CG.same(o["grad_src"], want_gs, label + ": grad_src")
        CG.same(o["grad_dst"], want_gd, label + ": grad_dst")

    CG.sweep(knobs, run, check, 0, "edge_dot_n2n dim %d" % F)
