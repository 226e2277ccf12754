"""The relation-typed edge score on the MI355X (wholegraph_amd/torch/kge_score.py -> csrc/kernels/kge.hip).

Scores and the three gradients are checked bit for bit against one numpy restatement of the order the header states
(include/wholememory/wholegraph_amd_ext.h, section 2u), built from the restatements the attention tests already hold
(tree_sum, seg_sum, per_source — the latter with the relation as the key for grad_rel), and on the random blocks with
assert_close_scaled against torch autograd in float64 through the plain composite at the tolerances of test_edge_dot_gpu.py
(1e-5 scores, 1e-4 gradients). Then every launch under a capped grid."""
import itertools

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
STEPS = {"distmult": ("mul", "dot"), "transe_l1": ("add", "l1"), "transe_l2": ("add", "l2"), "complex": ("cmul", "dot"),
         "rotate": ("cmul", "l2")}
MODELS = list(STEPS)
WIDTHS = [2, 6, 8, 64, 200, 256, 512]


def steps(model, h, r, t, g, xp):
    """(score, dh, dt, dr) of every edge from its rows, in the stated operations; xp concatenates, so that numpy (fp32, bit for
    bit) and torch (float64, under autograd) share the statement. g None: the score alone"""
    cmp, mea = STEPS[model]
    D = h.shape[1] // 2
    parts = (lambda x: [x[:, :D], x[:, D:]]) if cmp == "cmul" else (lambda x: [x])
    H, R, T = parts(h), parts(r), parts(t)
    U = {"mul": lambda: [H[0] * R[0]], "add": lambda: [H[0] + R[0]],
         "cmul": lambda: [H[0] * R[0] - H[1] * R[1], H[0] * R[1] + H[1] * R[0]]}[cmp]()
    Dd = [u - t_ for u, t_ in zip(U, T)]
    per_part = {"dot": lambda i: U[i] * T[i], "l1": lambda i: abs(Dd[i]), "l2": lambda i: Dd[i] * Dd[i]}[mea]
    term = per_part(0) if len(U) == 1 else per_part(0) + per_part(1)
    root = tree_sum(term) if xp is np else term.sum(-1)
    score = {"dot": lambda: root, "l1": lambda: -root, "l2": lambda: -xp.sqrt(root)}[mea]()
    if g is None:
        return score
    gg, n = g[:, None], (-score)[:, None]
    if mea == "dot":
        DU, DT = [gg * t_ for t_ in T], [gg * u for u in U]
    else:
        Q = [gg * np.sign(d) for d in Dd] if mea == "l1" else [np.where(n == 0, F32(0.0), gg * (d / n)) for d in Dd]
        DU, DT = [-q for q in Q], Q
    if cmp == "mul":
        DH, DR = [DU[0] * R[0]], [DU[0] * H[0]]
    elif cmp == "add":
        DH, DR = DU, DU
    else:
        DH = [DU[0] * R[0] + DU[1] * R[1], DU[1] * R[0] - DU[0] * R[1]]
        DR = [DU[0] * H[0] + DU[1] * H[1], DU[1] * H[0] - DU[0] * H[1]]
    return (score,) + tuple(xp.concatenate(p, 1) if xp is np else xp.cat(p, 1) for p in (DH, DT, DR))


def ref_all(model, head, row_ptr, col, et, xs, xd, rel, g, chunk):
    """(score, grad_src, grad_dst, grad_rel) in the stated order; a type outside [0, R): score and terms +0.0"""
    col, et = np.asarray(col, np.int64), np.asarray(et, np.int64)
    dst, R, n_dst = edge_dst(row_ptr), rel.shape[0], len(row_ptr) - 1
    ok = (et >= 0) & (et < R)
    own, far = xd[dst], xs[col]
    h, t = (own, far) if head == "dst" else (far, own)
    with np.errstate(all="ignore"):
        score, dh, dt, dr = steps(model, h, rel[np.where(ok, et, 0)], t, g, np)
    score, dh, dt, dr = (np.where(ok.reshape((-1,) + (1,) * (a.ndim - 1)), a, F32(0.0)).astype(F32) for a in (score, dh, dt, dr))
    d_own, d_far = (dh, dt) if head == "dst" else (dt, dh)
    gd = seg_sum(row_ptr, d_own) if n_dst else np.zeros((0, xs.shape[1]), F32)
    return score, per_source(col, xs.shape[0], d_far, chunk), gd, per_source(et, R, dr, chunk)


def composite64(model, head, xs, xd, rel, row_ptr, col, et):
    """float64 torch autograd through the same statement's forward"""
    import torch
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    own = xd.index_select(0, torch.repeat_interleave(torch.arange(deg.numel(), device=xs.device), deg))
    far = xs.index_select(0, col.long())
    h, t = (own, far) if head == "dst" else (far, own)
    return steps(model, h, rel.index_select(0, et.long()), t, None, torch)


def run_op(model, head, tensors, row_ptr, col, et, g_np, need=(True, True, True), index=np.int32):
    """(score, [grad_src, grad_dst, grad_rel]) of one forward + backward; a gradient is None where need is False"""
    from wholegraph_amd.torch.kge_score import kge_score_n2n
    xs, xd, rel = (t.detach().requires_grad_(n) for t, n in zip(tensors, need))
    rp, ci, ty = (dev(np.asarray(a, index)) for a in (row_ptr, col, et))
    score = kge_score_n2n(xs, xd, rel, rp, ci, ty, model=model, head=head)
    if any(need):
        score.backward(dev(g_np))
    return score.detach(), [xs.grad, xd.grad, rel.grad]


def same_bits(got, want):
    import torch
    for a, b in zip([got[0]] + list(got[1]), [want[0]] + list(want[1])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_all(model, head, xs, xd, rel, row_ptr, col, et, rng, loose=False, tensors=None):
    import torch
    from wholegraph_amd.torch.aggregation import chunk_edges
    n_dst = len(row_ptr) - 1
    g_np = rng.standard_normal(len(col)).astype(F32)
    score, grads = run_op(model, head, tensors or tuple(dev(a) for a in (xs, xd, rel)), row_ptr, col, et, g_np)
    want = ref_all(model, head, row_ptr, col, et, xs, xd[:n_dst], rel, g_np, chunk_edges())
    assert np.isfinite(want[0]).all() and all(bool(torch.isfinite(t).all()) for t in [score] + grads)
    assert np.array_equal(bits(score), want[0].view(np.uint32)), "score"
    assert np.array_equal(bits(grads[0]), want[1].view(np.uint32)), "grad_src"
    assert np.array_equal(bits(grads[1])[:n_dst], want[2].view(np.uint32)), "grad_dst"
    assert not grads[1][n_dst:].any()
    assert np.array_equal(bits(grads[2]), want[3].view(np.uint32)), "grad_rel"
    if loose:
        t64 = [dev(a.astype(np.float64)).requires_grad_(True) for a in (xs, xd, rel)]
        ref = composite64(model, head, *t64, dev(row_ptr), dev(col), dev(et))
        assert_close_scaled(score, ref.detach(), 1e-5)
        ref.backward(dev(g_np.astype(np.float64)))
        for got, t in zip(grads, t64):
            assert_close_scaled(got, t.grad)
    return score, grads, g_np


def rows(rng, n_src, n_dst, R, F):
    return tuple(rng.standard_normal((n, F)).astype(F32) for n in (n_src, n_dst, R))


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("model", MODELS)
def test_bitwise_on_random_and_hub_blocks(gpu_env, model, F):
    """real models: element-wise at 16 (2, 6) and 64 lanes (200, 512), the lane-split tree at 16 (8, 64: every lane of a group)
    and 64 lanes (256); complex models: element-wise at 16 lanes (2, 6: D % 4 != 0) and 64 (200), the 16-byte route with one
    lane (8) and with 8, 32 and 64 lanes (64, 256, 512). R = 1 on the hub block: one relation run of more than 2 C edges"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    rng = np.random.default_rng(4000 + F)
    row_ptr, col = block(rng, 300, 500, 12)
    et = rng.integers(0, 4, len(col)).astype(np.int32)   # (relation 4 of R = 5 has no edges)
    assert (np.diff(row_ptr) == 0).any() and (np.bincount(col, minlength=500) == 0).any() and (np.bincount(et, minlength=5) == 0).any()
    check_all(model, "dst", *rows(rng, 500, 300, 5, F), row_ptr, col, et, rng, loose=True)
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    assert len(col) > 2 * chunk_edges()
    check_all(model, "dst", *rows(rng, n_src, n_dst, 1, F), row_ptr, col, np.zeros(len(col), np.int32), rng)


@pytest.mark.parametrize("F", [6, 8])
@pytest.mark.parametrize("model", MODELS)
def test_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, model, F):
    from wholegraph_amd.torch.aggregation import chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(4100 + F)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    et = (np.arange(len(col)) % 3).astype(np.int32)
    assert len(col) // 3 > 9 * C   # more than one batch of partial rows per relation too
    check_all(model, "dst", *rows(rng, LR.N_SRC, LR.N_DST, 3, F), row_ptr, col, et, rng)


@pytest.mark.parametrize("head", ["dst", "src"])
@pytest.mark.parametrize("model", MODELS)
def test_both_heads_degree_70_more_targets_than_sources_more_relations_than_edges(gpu_env, model, head):
    rng = np.random.default_rng(4200)
    n_dst, n_src, R = 30, 20, 200
    deg = rng.integers(0, 4, n_dst)
    deg[3] = 70
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    E = int(row_ptr[-1])
    assert R > E
    col = rng.integers(0, n_src, E).astype(np.int32)
    et = rng.integers(0, R, E).astype(np.int32)
    for F in (6, 32):
        check_all(model, head, *rows(rng, n_src, n_dst, R, F), row_ptr, col, et, rng, loose=True)


@pytest.mark.parametrize("model", MODELS)
def test_types_out_of_range_and_planted_zeros(gpu_env, model):
    """edge 0 has type -1 and edge 1 type R: score +0.0, no gradient. Edge 2 has u == t in every column (the l2 models: n == 0,
    every q +0.0; l1: sgn(0) = 0), edge 3 in column 0 only; dyadic values, so the zeros are exact"""
    rng = np.random.default_rng(4300)
    R, F = 3, 8
    row_ptr, col = np.array([0, 3, 6], np.int32), np.array([0, 1, 2, 3, 4, 0], np.int32)
    et = np.array([-1, R, 1, 2, 0, 1], np.int32)
    xs, xd, rel = rows(rng, 5, 2, R, F)
    xd[:], rel[1], rel[2] = 0.5, 0.25, 0.75
    cmp = STEPS[model][0]
    u1 = {"mul": 0.125, "add": 0.75, "cmul": 0.0}[cmp]   # 0.5 (x) 0.25: the real part of (.5 + .5i)(.25 + .25i) is 0
    xs[2] = u1
    if cmp == "cmul":
        xs[2, F // 2:] = 0.25
    xs[3, 0] = {"mul": 0.375, "add": 1.25, "cmul": 0.0}[cmp]
    score, grads, _ = check_all(model, "dst", xs, xd, rel, row_ptr, col, et, rng)
    assert not bits(score)[:2].any()
    if STEPS[model][1] != "dot":
        assert float(score[2]) == 0.0


@pytest.mark.parametrize("model", MODELS)
def test_empty_blocks(gpu_env, model):
    rng = np.random.default_rng(4400)
    for n_dst in (0, 6):   # n_dst = 0, then E = 0 with targets
        score, grads, _ = check_all(model, "dst", *rows(rng, 50, n_dst, 4, 8), np.zeros(n_dst + 1, np.int32),
                                    np.zeros(0, np.int32), np.zeros(0, np.int32), rng)
        assert score.numel() == 0
        assert all(np.array_equal(bits(g), np.zeros(g.shape, np.uint32)) for g in grads)   # +0.0


@pytest.mark.parametrize("model", MODELS)
def test_gradient_subsets_int64_indices_and_misaligned_views(gpu_env, model):
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col, n_dst, n_src = hub_block(chunk_edges())
    rng = np.random.default_rng(4500)
    R, F = 4, 32
    et = rng.integers(0, R, len(col)).astype(np.int32)
    wide = [rng.standard_normal((n, F + 9)).astype(F32) for n in (n_src, n_dst + 3, R)]
    t = tuple(dev(w[:, 1:1 + F].copy()) for w in wide)
    g = rng.standard_normal(len(col)).astype(F32)
    full = run_op(model, "dst", t, row_ptr, col, et, g)
    same_bits(run_op(model, "dst", t, row_ptr, col, et, g, index=np.int64), full)
    views = tuple(dev(w)[:, 1:1 + F] for w in wide)   # one element off 16-byte alignment: the element-wise routes
    assert all(v.data_ptr() % 16 != 0 and v.stride(0) > F for v in views)
    same_bits(run_op(model, "dst", views, row_ptr, col, et, g), full)
    for need in itertools.product((False, True), repeat=3):
        score, grads = run_op(model, "dst", t, row_ptr, col, et, g, need)
        assert [x is not None for x in grads] == list(need)
        same_bits((score, [a for a in grads if a is not None]), (full[0], [b for a, b in zip(grads, full[1]) if a is not None]))


def test_refusals(gpu_env):
    import torch
    from wholegraph_amd.torch.kge_score import kge_score_n2n
    rng = np.random.default_rng(4600)
    row_ptr, col = block(rng, 20, 30, 5)
    rp, ci, ty = dev(row_ptr), dev(col), dev(np.zeros(len(col), np.int32))
    xs, xd, rel = (dev(a) for a in rows(rng, 30, 20, 2, 7))
    with pytest.raises(ValueError, match="even"):
        kge_score_n2n(xs, xd, rel, rp, ci, ty, model="rotate")
    with pytest.raises(TypeError, match="float32"):
        kge_score_n2n(xs.bfloat16(), xd, rel, rp, ci, ty, model="distmult")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        score = kge_score_n2n(xs.bfloat16(), xd, rel, rp, ci, ty, model="distmult")
    want = kge_score_n2n(xs.bfloat16().float(), xd, rel, rp, ci, ty, model="distmult")
    assert score.dtype == torch.float32 and torch.equal(score.view(torch.int32), want.view(torch.int32))


# launch sites: kge_fwd_kernel and kge_bwd_dst_kernel (301 targets), agg_bwd_prep_kernel twice (one thread per edge),
# kge_bwd_chunk_kernel twice (21 tiles), kge_bwd_fold_kernel over 1103 sources and over 40 relations (3 workgroups of 16
# groups). Each wants more than one workgroup at every width: full = 0. Relation 0 holds every second edge: a run of chunks.
@pytest.mark.parametrize("model,F", [(m, F) for m in MODELS for F in CG.WIDTHS if F % 2 == 0 or STEPS[m][0] != "cmul"])
def test_under_a_capped_grid(gpu_env, knobs, model, F):
    C_, row_ptr, col = CG.the_block()
    rng = np.random.default_rng(4700 + F)
    R = 40
    et = np.where(np.arange(len(col)) % 2 == 0, 0, rng.integers(1, R, len(col))).astype(np.int32)
    arrays = rows(rng, CB.N_SRC, CB.N_DST, R, F)
    g_np = rng.standard_normal(len(col)).astype(F32)
    names = ("score", "grad_src", "grad_dst", "grad_rel")
    want = ref_all(model, "dst", row_ptr, col, et, *arrays, g_np, C_)

    def run(other):
        from wholegraph_amd.torch.kge_score import kge_score_n2n
        xs, xd, rel = (CG.dev(CG.alt(a, other)).requires_grad_(True) for a in arrays)
        score = kge_score_n2n(xs, xd, rel, CG.dev(row_ptr), CG.dev(col), CG.dev(et), model=model)
        score.backward(CG.dev(CG.alt(g_np, other)))
        return dict(zip(names, (CG.np_of(t) for t in (score, xs.grad, xd.grad, rel.grad))))

    def check(o, label):
        for name, w in zip(names, want):
            CG.same(o[name], w, "%s: %s" % (label, name))

    CG.sweep(knobs, run, check, 0, "kge_score_n2n %s dim %d" % (model, F))
