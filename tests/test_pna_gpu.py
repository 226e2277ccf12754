"""Multi-aggregator neighbour aggregation on the MI355X (wholegraph_amd/torch/pna_aggregation.py -> csrc/kernels/pna.hip).

Forward, the buffers saved for the backward, and the backward are checked bit for bit against a numpy restatement of the
order the header states (include/wholememory/wholegraph_amd_ext.h, section 2l); the sum and mean slots against agg_concat;
everything against torch autograd through a float64 index_select / scatter_reduce / index_add_ composite on inputs without
ties, each element within the worst-case error bound of the stated fp32 arithmetic. Then the mechanical cases (views,
int64 indices, empty blocks, no_grad), PNAConv against a hand-built composite, and a two-layer "pna" HomoGNNModel trained
end to end on a planted-partition graph held in WholeMemory.

The blocks are the smallest that reach every path: F = 1 and 3 (scalar path), 4, 64, 128 (16-byte path at 16 and 32 lanes)
and 260 (64 lanes and a second column pass); degrees 0, 1, 8, 9, 16, 17, 64, 65 (batch and group boundaries) and 300 (several
loads of column ids); about 44 targets among 200 sources, sources without edges on both sides of n_dst, and one hub whose
run of about 1200 edges has three chunks."""
import functools
import random
import types

import numpy as np
import pytest

from test_sage_agg_gpu import _planted_partition, _wm_array, bits, dev

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of fp32
EPS = F32(1e-5)
ORDER = ("sum", "mean", "min", "max", "std")
DIMS = [1, 3, 4, 64, 128, 260]
MASKS = [ORDER, ("max",), ("min", "std"), ("sum", "mean")]
DEGREES = (0, 1, 8, 9, 16, 17, 64, 65)
N_SRC, HUB = 200, 3


def slots_of(names):
    names = [n for n in ORDER if n in names]
    return {n: i for i, n in enumerate(names)}, len(names)


# ---------------------------------------------------------------- the order, restated
def ref_forward(row_ptr, col, x, names, eps=EPS):
    """(out, saved) in the stated order: S and Q left to right from the first term, min / max replaced on a strict
    comparison only, m = S r, v = Q r - m m, std = sqrt(max(v, 0) + eps), c = r / std where v > 0; +0.0 and arg -1 for an
    empty target. saved: arg_min, arg_max, std_mean, std_coef (None when not selected)"""
    row_ptr = np.asarray(row_ptr, np.int64)
    n_dst, F = len(row_ptr) - 1, x.shape[1]
    deg = np.diff(row_ptr)
    S, Q = np.zeros((n_dst, F), F32), np.zeros((n_dst, F), F32)
    mn, mx = np.zeros((n_dst, F), F32), np.zeros((n_dst, F), F32)
    amin, amax = np.full((n_dst, F), -1, np.int32), np.full((n_dst, F), -1, np.int32)
    for k in range(int(deg.max()) if n_dst else 0):   # k-th term of every target that has one: same order per target
        live = np.nonzero(deg > k)[0]
        e = (row_ptr[live] + k).astype(np.int32)
        t = x[col[e]]
        sq = t * t
        if k == 0:
            S[live], Q[live], mn[live], mx[live] = t, sq, t, t
            amin[live], amax[live] = e[:, None], e[:, None]
            continue
        S[live] = S[live] + t
        Q[live] = Q[live] + sq
        lo, hi = t < mn[live], t > mx[live]
        mn[live] = np.where(lo, t, mn[live])
        mx[live] = np.where(hi, t, mx[live])
        amin[live] = np.where(lo, e[:, None], amin[live])
        amax[live] = np.where(hi, e[:, None], amax[live])
    any_ = (deg > 0)[:, None]
    r = np.where(deg > 0, F32(1.0) / np.maximum(deg, 1).astype(F32), F32(0.0)).astype(F32)[:, None]
    m = (S * r).astype(F32)
    v = ((Q * r).astype(F32) - (m * m).astype(F32)).astype(F32)
    sd = np.sqrt((np.where(v > 0, v, F32(0.0)).astype(F32) + F32(eps)).astype(F32)).astype(F32)
    c = np.where(v > 0, (r / sd).astype(F32), F32(0.0)).astype(F32)
    zero = np.zeros((n_dst, F), F32)
    slot = {"sum": np.where(any_, S, zero), "mean": np.where(any_, m, zero), "min": mn, "max": mx,
            "std": np.where(any_, sd, zero)}
    out = np.concatenate([slot[n] for n in ORDER if n in names] + [x[:n_dst]], axis=1).astype(F32)
    saved = (amin if "min" in names else None, amax if "max" in names else None,
             np.where(any_, m, zero) if "std" in names else None, np.where(any_, c, zero) if "std" in names else None)
    return out, saved


def ref_backward(row_ptr, col, x, names, saved, G, chunk):
    """grad_x in the stated order: the parts of an edge's term added in slot order from the first one present, the terms of a
    source from +0.0 in ascending edge position within chunks, the chunk sums in chunk order, the self term last"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, n_src, F = len(row_ptr) - 1, x.shape[0], x.shape[1]
    slot, A = slots_of(names)
    deg = np.diff(row_ptr)
    dst = np.repeat(np.arange(n_dst), deg)
    E = len(col)
    pos = np.arange(E, dtype=np.int32)[:, None]
    amin, amax, m, c = saved
    part = lambda n: G[dst, slot[n] * F:(slot[n] + 1) * F]
    t = np.full((E, F), -0.0, F32)   # (-0.0 + a part is that part; a term that stays -0.0 adds nothing to a sum from +0.0)
    if "sum" in names:
        t = t + part("sum")
    if "mean" in names:
        t = t + (part("mean") * (F32(1.0) / deg[dst].astype(F32))[:, None]).astype(F32)
    if "min" in names:
        t = np.where(amin[dst] == pos, t + part("min"), t)
    if "max" in names:
        t = np.where(amax[dst] == pos, t + part("max"), t)
    if "std" in names:
        t = t + ((part("std") * c[dst]).astype(F32) * (x[col] - m[dst]).astype(F32)).astype(F32)
    t = t.astype(F32)
    gx = np.zeros((n_src, F), F32)
    order = np.argsort(col, kind="stable")
    starts = np.searchsorted(col[order], np.arange(n_src + 1))
    for s in range(n_src):
        edges = order[starts[s]:starts[s + 1]]
        p = None
        for c0 in range(0, len(edges), chunk):
            pp = np.zeros(F, F32)
            for e in edges[c0:c0 + chunk]:
                pp = pp + t[e]
            p = pp if p is None else p + pp
        if s < n_dst:
            gx[s] = G[s, A * F:] if p is None else p + G[s, A * F:]
        elif p is not None:
            gx[s] = p
    return gx


# ---------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def ladder_block():
    """row_ptr, col: five targets of every degree of the ladder and four of degree 300 that hold only the hub; ids drawn
    from the even sources (the odd ones, the hub aside, have no edge), so duplicate edges are common, and forced where the
    degree allows"""
    rng = np.random.default_rng(5)
    deg = np.array(list(DEGREES) * 5 + [300] * 4)
    perm = rng.permutation(len(deg))
    deg = deg[perm]
    row_ptr = np.zeros(len(deg) + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = (2 * rng.integers(0, N_SRC // 2, int(row_ptr[-1]))).astype(np.int32)
    col[rng.random(len(col)) < 0.05] = HUB
    for d in np.nonzero(deg == 300)[0]:
        col[row_ptr[d]:row_ptr[d + 1]] = HUB
    for d in np.nonzero((deg >= 8) & (deg < 300))[0]:
        col[row_ptr[d] + 1] = col[row_ptr[d]]                    # the first edge twice
        col[row_ptr[d + 1] - 1] = col[row_ptr[d] + 3]            # and one more pair
    return row_ptr, col


def ladder_rows(F):
    """x [N_SRC, F]: standard normal, with column 0 the constant 2 (F > 1) and column 1 drawn from -0.0, +0.0 and 1"""
    rng = np.random.default_rng(100 + F)
    x = rng.standard_normal((N_SRC, F)).astype(F32)
    if F > 1:
        x[:, 0] = 2.0
        x[:, 1] = rng.choice(np.array([-0.0, 0.0, 1.0], F32), N_SRC)
    return x


@functools.lru_cache(maxsize=None)
def ladder_case(F, names):
    """the inputs of one (F, aggregators) case and its reference, computed once"""
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col = ladder_block()
    x = ladder_rows(F)
    A = len(names)
    G = np.random.default_rng(7 * F + A).standard_normal((len(row_ptr) - 1, (A + 1) * F)).astype(F32)
    out, saved = ref_forward(row_ptr, col, x, names)
    gx = ref_backward(row_ptr, col, x, names, saved, G, chunk_edges())
    return row_ptr, col, x, G, out, saved, gx


def run_op(x, row_ptr, col, names, G):
    """(out, saved tensors of the backward, grad_x) of the op on numpy inputs"""
    import torch
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    xt = dev(x).requires_grad_(True)
    out = agg_concat_pna(xt, dev(row_ptr), dev(col), list(names))
    saved = out.grad_fn.saved_tensors[3:]
    (gx,) = torch.autograd.grad(out, xt, dev(G))
    return out, saved, gx


def test_the_ladder_block_keeps_its_point(gpu_env):
    from wholegraph_amd.torch.aggregation import chunk_edges
    row_ptr, col = ladder_block()
    C = chunk_edges()
    deg = np.diff(row_ptr)
    assert set(DEGREES) | {300} == set(deg.tolist()) and len(deg) == 44
    counts = np.bincount(col, minlength=N_SRC)
    assert 2 * C < counts[HUB] <= 3 * C                      # the hub's run has three chunks
    assert (counts[:44] == 0).any() and (counts[44:] == 0).any()
    assert all(col[row_ptr[d]] == col[row_ptr[d] + 1] for d in np.nonzero((deg >= 8) & (deg < 300))[0])
    x = ladder_rows(4)
    _, (_, _, m, c) = ref_forward(row_ptr, col, x, ORDER)
    pow2 = np.isin(deg, (1, 8, 16, 64))                       # r is exact there: the constant column has v = 0 exactly
    assert (c[pow2, 0] == 0).all() and (m[pow2, 0] == 2).all()
    assert np.signbit(x[:, 1]).any() and (x[:, 1] == 0).sum() > np.signbit(x[:, 1]).sum()


# ---------------------------------------------------------------- 1 bit for bit
@pytest.mark.parametrize("F", DIMS)
@pytest.mark.parametrize("names", MASKS, ids="-".join)
def test_forward_saved_and_backward_bitwise(gpu_env, F, names):
    row_ptr, col, x, G, want_out, want_saved, want_gx = ladder_case(F, names)
    out, saved, gx = run_op(x, row_ptr, col, names[::-1], G)   # (listed backwards: the slots keep the canonical order)
    assert out.shape == want_out.shape
    assert np.array_equal(bits(out), want_out.view(np.uint32))
    for got, want, what in zip(saved, want_saved, ("arg_min", "arg_max", "std_mean", "std_coef")):
        assert (got is None) == (want is None), what
        if want is not None:
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), what
    assert np.array_equal(bits(gx), want_gx.view(np.uint32))
    if "std" in names and F > 1:   # the constant column on a target with an exact r: std = sqrt(eps), no gradient through it
        deg = np.diff(row_ptr)
        d = int(np.nonzero(deg == 8)[0][0])
        slot, _ = slots_of(names)
        assert bits(out)[d, slot["std"] * F] == np.sqrt(EPS).view(np.uint32)
        assert want_saved[3][d, 0] == 0


# ---------------------------------------------------------------- 2 against agg_concat
@pytest.mark.parametrize("F", DIMS)
def test_sum_and_mean_slots_are_agg_concat(gpu_env, F):
    from wholegraph_amd.torch.aggregation import agg_concat
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    row_ptr, col = ladder_block()
    x, rp, ci = dev(ladder_rows(F)), dev(row_ptr), dev(col)
    n_dst = len(row_ptr) - 1
    out = agg_concat_pna(x, rp, ci, ORDER)
    assert np.array_equal(bits(out[:, :F]), bits(agg_concat(x, rp, ci, "sum")[:, :F]))
    assert np.array_equal(bits(out[:, F:2 * F]), bits(agg_concat(x, rp, ci, "mean")[:, :F]))
    assert np.array_equal(bits(out[:, 5 * F:]), bits(x[:n_dst]))
    only = agg_concat_pna(x, rp, ci, ["max"])
    assert np.array_equal(bits(only), bits(out[:, [*range(3 * F, 4 * F), *range(5 * F, 6 * F)]]))


# ---------------------------------------------------------------- 3 against torch autograd
def composite(x, row_ptr, col, names, eps=1e-5):
    """torch autograd reference in x's dtype: index_select, index_add_ and scatter_reduce (amin / amax), PyG's std; a target
    without edges gets 0 in every slot, as the op"""
    import torch
    n_dst, F = row_ptr.numel() - 1, x.shape[1]
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n_dst, device=x.device), deg)
    xe = x.index_select(0, col.long())
    zero = torch.zeros((n_dst, F), device=x.device, dtype=x.dtype)
    n = deg.clamp(min=1).to(x.dtype)[:, None]
    idx = dst[:, None].expand(-1, F)
    S = zero.index_add(0, dst, xe)
    res = {"sum": S, "mean": S / n}
    if "min" in names:
        res["min"] = zero.scatter_reduce(0, idx, xe, "amin", include_self=False)
    if "max" in names:
        res["max"] = zero.scatter_reduce(0, idx, xe, "amax", include_self=False)
    if "std" in names:
        var = zero.index_add(0, dst, xe * xe) / n - res["mean"] * res["mean"]
        res["std"] = (var.relu() + eps).sqrt() * (deg > 0).to(x.dtype)[:, None]
    return torch.cat([res[k] for k in ORDER if k in names] + [x[:n_dst]], dim=1)


def tie_free_block(rng, n_dst, n_src):
    """the degree ladder with distinct neighbours per target (no duplicate edges), and a source in every target"""
    deg = rng.permutation(np.array(list(DEGREES) * (n_dst // len(DEGREES))))
    row_ptr = np.zeros(len(deg) + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = np.concatenate([rng.choice(n_src, d, replace=False) for d in deg]).astype(np.int32)
    return row_ptr, col


def error_bounds(row_ptr, col, x, names, G):
    """worst-case error of the stated fp32 arithmetic, per element, from float64 magnitudes (u = 2^-24; a left-to-right sum
    of n terms errs by at most (n - 1) u sum|t|, every other operation by u times its result, first order in u):
    forward [n_dst, A * F] and grad_x [n_src, F]"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    x = x.astype(np.float64)
    G = G.astype(np.float64)
    n_dst, n_src, F = len(row_ptr) - 1, x.shape[0], x.shape[1]
    slot, A = slots_of(names)
    deg = np.diff(row_ptr)
    dst = np.repeat(np.arange(n_dst), deg)
    n = np.maximum(deg, 1).astype(np.float64)[:, None]
    seg = lambda t: np.add.reduceat(np.concatenate([t, np.zeros((1, F))]), np.minimum(row_ptr[:-1], len(t))) * (deg > 0)[:, None]
    a1, a2, s1 = seg(np.abs(x[col])), seg(x[col] ** 2), seg(x[col])
    mean = s1 / n
    e_sum = n * U * a1                                   # S
    e_mean = (n + 2) * U * a1 / n                        # S * fl(1 / n): r and the product round as well
    var = np.maximum(a2 / n - mean ** 2, 0)
    std = np.sqrt(var + 1e-5)
    # Q (squares rounded, then summed) times r; m * m from m's error; the subtraction
    e_var = (n + 3) * U * a2 / n + 2 * np.abs(mean) * e_mean + U * mean ** 2 + U * var
    e_std = e_var / (2 * std) + 2 * U * std              # the addition of eps and the square root round too
    fwd = np.zeros((n_dst, A * F))
    for name, e in (("sum", e_sum), ("mean", e_mean), ("std", e_std)):
        if name in names:
            fwd[:, slot[name] * F:(slot[name] + 1) * F] = e
    # an edge's term: the magnitudes of its parts, and what the std part inherits from m, c and std
    part = lambda k: np.abs(G[dst, slot[k] * F:(slot[k] + 1) * F])
    mag = np.zeros((len(col), F))
    extra = np.zeros((len(col), F))
    for name in ("sum", "min", "max"):
        if name in names:
            mag += part(name)                             # (min / max: at most this much, where the edge is the arg)
    if "mean" in names:
        mag += part("mean") / n[dst]
    if "std" in names:
        c = 1 / (n * std)
        dev_ = np.abs(x[col] - mean[dst])
        mag += part("std") * c[dst] * dev_
        extra = part("std") * (c[dst] * (e_mean[dst] + U * dev_) + c[dst] * dev_ * (4 * U + e_std[dst] / std[dst]))
    T = np.zeros((n_src, F))
    X = np.zeros((n_src, F))
    np.add.at(T, col, mag)
    np.add.at(X, col, extra)
    T[:n_dst] += np.abs(G[:, A * F:])
    counts = np.bincount(col, minlength=n_src).astype(np.float64)[:, None]
    bwd = (counts + 1 + 8) * U * T + X                    # the sum over the edges and the self term; 4 adds and 4 products a term
    return fwd, bwd


@pytest.mark.parametrize("F", [3, 64])
@pytest.mark.parametrize("names", MASKS, ids="-".join)
def test_against_float64_autograd(gpu_env, F, names):
    """Standard-normal rows: the variance of a target's neighbours is then of the order of E[x^2], so v = Q r - m^2 does not
    cancel and the bound of std (which divides the error of v by 2 std) stays a few u; near-constant columns are the
    bitwise test's business."""
    import torch
    rng = np.random.default_rng(31 + F)
    n_dst, n_src = 40, N_SRC
    row_ptr, col = tie_free_block(rng, n_dst, n_src)
    x = rng.standard_normal((n_src, F)).astype(F32)
    A = len(names)
    G = rng.standard_normal((n_dst, (A + 1) * F)).astype(F32)
    # the composite's amin / amax backward splits a gradient among ties, the op gives it to the first edge: no ties here
    assert all(len(np.unique(col[row_ptr[d]:row_ptr[d + 1]])) == row_ptr[d + 1] - row_ptr[d] for d in range(n_dst))
    assert all(len(np.unique(x[:, f])) == n_src for f in range(F))
    out, _, gx = run_op(x, row_ptr, col, names, G)
    x64 = dev(x.astype(np.float64)).requires_grad_(True)
    want = composite(x64, dev(row_ptr), dev(col), names)
    (want_gx,) = torch.autograd.grad(want, x64, dev(G.astype(np.float64)))
    fwd_bound, bwd_bound = error_bounds(row_ptr, col, x, names, G)
    slot, _ = slots_of(names)
    got, want = out.detach().double().cpu().numpy(), want.detach().cpu().numpy()
    for name in ("min", "max"):
        if name in names:
            cols = slice(slot[name] * F, (slot[name] + 1) * F)
            assert np.array_equal(got[:, cols], want[:, cols]), name
    assert np.array_equal(got[:, A * F:], want[:, A * F:])
    diff = np.abs(got[:, :A * F] - want[:, :A * F])
    excess = diff - (1e-5 * np.abs(want[:, :A * F]) + fwd_bound + 1e-7)
    print("forward: max |diff| %.3g, max bound %.3g" % (diff.max(), fwd_bound.max()))
    assert (excess <= 0).all(), "max excess %g" % excess.max()
    diff = np.abs(gx.double().cpu().numpy() - want_gx.cpu().numpy())
    excess = diff - (1e-5 * np.abs(want_gx.cpu().numpy()) + bwd_bound + 1e-7)
    print("backward: max |diff| %.3g, max bound %.3g" % (diff.max(), bwd_bound.max()))
    assert (excess <= 0).all(), "max excess %g" % excess.max()


# ---------------------------------------------------------------- 4 mechanical cases
def test_views_and_int64_indices_give_the_same_bits(gpu_env):
    import torch
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    F = 64
    row_ptr, col, x, G, want_out, _, want_gx = ladder_case(F, ORDER)
    rp, ci, g = dev(row_ptr), dev(col), dev(G)
    wide = torch.zeros((N_SRC, F + 8), device="cuda")
    views = {"misaligned": wide[:, 1:F + 1], "strided": wide[:, 4:F + 4], "odd stride": torch.zeros((N_SRC, F + 3), device="cuda")[:, :F]}
    for what, view in views.items():
        view.copy_(dev(x))
        assert not view.is_contiguous()
        xt = view.detach().requires_grad_(True)
        out = agg_concat_pna(xt, rp, ci, ORDER)
        assert np.array_equal(bits(out), want_out.view(np.uint32)), what
        # grad_out as a view of the same kind
        goff = 4 if what == "strided" else 1
        gwide = torch.zeros((g.shape[0], g.shape[1] + 8), device="cuda")
        gwide[:, goff:g.shape[1] + goff] = g
        (gx,) = torch.autograd.grad(out, xt, gwide[:, goff:g.shape[1] + goff])
        assert np.array_equal(bits(gx), want_gx.view(np.uint32)), what
    xt = dev(x).requires_grad_(True)
    out = agg_concat_pna(xt, dev(row_ptr.astype(np.int64)), dev(col.astype(np.int64)), ORDER)
    (gx,) = torch.autograd.grad(out, xt, g)
    assert np.array_equal(bits(out), want_out.view(np.uint32)) and np.array_equal(bits(gx), want_gx.view(np.uint32))


@pytest.mark.parametrize("F", [3, 8])
def test_empty_blocks(gpu_env, F):
    import torch
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    x = np.random.default_rng(F).standard_normal((7, F)).astype(F32)
    none = np.zeros(0, np.int32)
    # no target at all
    xt = dev(x).requires_grad_(True)
    out = agg_concat_pna(xt, dev(np.zeros(1, np.int32)), dev(none), ORDER)
    assert out.shape == (0, 6 * F)
    (gx,) = torch.autograd.grad(out.sum(), xt)
    assert not bits(gx).any()
    # targets, none with an edge (n_edges = 0, and a block of only empty targets): +0.0 and the own row, arg -1
    for names in MASKS:
        A = len(names)
        xt = dev(x).requires_grad_(True)
        out = agg_concat_pna(xt, dev(np.zeros(5, np.int32)), dev(none), names)
        assert not bits(out[:, :A * F]).any() and np.array_equal(bits(out[:, A * F:]), x[:4].view(np.uint32))
        for t, dt in zip(out.grad_fn.saved_tensors[3:], (torch.int32, torch.int32, torch.float32, torch.float32)):
            if t is not None:
                assert t.dtype == dt and bool((t == (-1 if dt == torch.int32 else 0)).all())
        G = np.random.default_rng(9).standard_normal((4, (A + 1) * F)).astype(F32)
        (gx,) = torch.autograd.grad(out, xt, dev(G))
        assert np.array_equal(bits(gx[:4]), G[:, A * F:].view(np.uint32)) and not bits(gx[4:]).any()


def test_no_grad_allocates_no_saved_buffer_and_calls_repeat(gpu_env, monkeypatch):
    import torch
    from wholegraph_amd.torch import pna_aggregation as pa
    row_ptr, col, x, G, want_out, _, want_gx = ladder_case(64, ORDER)
    rp, ci = dev(row_ptr), dev(col)
    calls = []
    real = pa.wmb.lib()

    class Lib:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "wholememory_ext_csc_pna_aggregate_forward":
                return fn
            return lambda *a: (calls.append(a[12:16]), fn(*a))[1]

    monkeypatch.setattr(pa, "wmb", types.SimpleNamespace(lib=lambda: Lib(), check=pa.wmb.check, PNA_AGGR=pa.wmb.PNA_AGGR))
    xt = dev(x).requires_grad_(True)
    with torch.no_grad():
        quiet = pa.agg_concat_pna(xt, rp, ci, ORDER)
    plain = pa.agg_concat_pna(dev(x), rp, ci, ORDER)          # nothing to differentiate
    loud = pa.agg_concat_pna(xt, rp, ci, ORDER)
    part = pa.agg_concat_pna(xt, rp, ci, ["sum", "max"])
    assert calls[0] == (None,) * 4 and calls[1] == (None,) * 4
    assert all(p is not None for p in calls[2])
    assert [p is not None for p in calls[3]] == [False, True, False, False]   # only what a selected aggregator needs
    assert quiet.grad_fn is None and plain.grad_fn is None
    for t in (quiet, plain, loud):
        assert np.array_equal(bits(t), want_out.view(np.uint32))
    # two identical calls give identical bits, forward and backward
    (gx1,) = torch.autograd.grad(loud, xt, dev(G))
    (gx2,) = torch.autograd.grad(pa.agg_concat_pna(xt, rp, ci, ORDER), xt, dev(G))
    assert np.array_equal(bits(gx1), bits(gx2)) and np.array_equal(bits(gx1), want_gx.view(np.uint32))


# ---------------------------------------------------------------- 5 the layer
def layer_reference(layer, x, row_ptr, col):
    """PNAConv from its own parameters over the composite"""
    import torch
    h = torch.relu(layer.pre_lin(x)) if layer.pre_lin is not None else x
    agg = composite(h.float(), row_ptr, col, layer.aggregators)
    width = len(layer.aggregators) * layer.in_channels
    stats, own = agg[:, :width], agg[:, width:]
    deg = (row_ptr[1:] - row_ptr[:-1]).float()
    logd = torch.log(deg + 1)[:, None]
    scale = {"identity": torch.ones_like(logd), "amplification": logd / (layer.delta or 1.0),
             "attenuation": torch.where(deg[:, None] > 0, (layer.delta or 1.0) / logd.clamp(min=1e-30), torch.zeros_like(logd))}
    blocks = [stats * scale[s] for s in layer.scalers] + ([own] if layer.root_weight else [])
    return layer.lin(torch.cat(blocks, dim=1))


@pytest.mark.parametrize("project", [False, True])
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("scalers", [("identity",), ("amplification",), ("attenuation",),
                                     ("identity", "amplification", "attenuation")], ids="-".join)
def test_pna_conv_matches_composite(gpu_env, project, root, scalers):
    """fp32: the layer's last Linear sums at most 13 * 24 products of magnitudes of order 1, and the op differs from the
    composite by the order of fp32 sums: rtol = atol = 1e-4 is some 50 times the worst case of those sums. Under bf16 autocast
    both sides feed the same widened rows to the aggregation, and the Linear behind it rounds its output to bf16 (8
    significant bits): a difference of one unit in the last place of the largest outputs, 2^-7 of their magnitude."""
    import torch
    from wholegraph_amd.torch.cugraphops import PNAConv, pna_delta
    from test_sage_agg_gpu import block
    torch.manual_seed(4)
    rng = np.random.default_rng(41)
    n_dst, n_src, cin, cout = 60, 300, 24, 10
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    delta = pna_delta(rp)
    assert abs(delta - np.log(np.diff(row_ptr) + 1.0).mean()) < 1e-12
    layer = PNAConv(cin, cout, scalers=scalers, delta=delta, project=project, root_weight=root).cuda()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    out = layer(x, rp, ci, 20)
    ref = layer_reference(layer, x, rp, ci)
    assert out.shape == (n_dst, cout) and out.dtype == torch.float32
    assert torch.allclose(out, ref, rtol=1e-4, atol=1e-4), float((out - ref).detach().abs().max())
    # gradients: of the last Linear always; of x and pre_lin only without the projection, whose relu zeros tie in min / max
    # (the composite splits a gradient among ties, the op gives it to the first edge)
    params = dict(layer.named_parameters())
    names = sorted(n for n in params if project is False or n.startswith("lin."))
    wrt = ([] if project else [x]) + [params[n] for n in names]
    got = torch.autograd.grad(out.square().sum(), wrt)
    want = torch.autograd.grad(ref.square().sum(), wrt)
    for g, w in zip(got, want):
        scale = float(w.abs().max())
        assert scale > 0 and torch.allclose(g, w, rtol=1e-4, atol=1e-4 * scale), float((g - w).abs().max())
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = layer(x, rp, ci, 20)
        ref16 = layer_reference(layer, x, rp, ci)
    assert out16.dtype == torch.bfloat16
    scale = float(ref16.detach().float().abs().max())
    assert torch.allclose(out16.float(), ref16.float(), rtol=2.0 ** -7, atol=2.0 ** -7 * scale)
    out16.float().sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().sum()) > 0


def test_autocast_rule_of_the_op(gpu_env):
    import torch
    from wholegraph_amd.torch.pna_aggregation import agg_concat_pna
    row_ptr, col = ladder_block()
    rp, ci = dev(row_ptr), dev(col)
    x = dev(ladder_rows(64))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = agg_concat_pna(x.bfloat16(), rp, ci)
        same = agg_concat_pna(x, rp, ci)                         # fp32 rows stay fp32 rows
    assert out.dtype == torch.float32
    assert np.array_equal(bits(out), bits(agg_concat_pna(x.bfloat16().float(), rp, ci)))
    assert np.array_equal(bits(same), bits(agg_concat_pna(x, rp, ci)))
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            agg_concat_pna(x.to(dt), rp, ci)


# ---------------------------------------------------------------- 6 end to end
def train_pna(comm, seed, with_composite=False):
    """a 2-layer "pna" HomoGNNModel on the planted-partition graph of the other end-to-end tests: the losses, the accuracy,
    the share of embedding rows that moved and the final evaluation logits. with_composite: the op replaced by the torch
    composite above (the reference run the bars were checked against)"""
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import pna_conv
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
    sampled = np.concatenate([[0], np.minimum(np.diff(row_ptr), 10).cumsum()])   # (degrees as the sampler cuts them: <= 10)
    delta = pna_conv.pna_delta(torch.from_numpy(sampled))
    args = types.SimpleNamespace(model="pna", hiddensize=64, layernum=2, classnum=k, dropout=0.1, neighbors="10,10",
                                 inferencesample="10,10", pna_delta=delta)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    assert [type(l).__name__ for l in model.gnn_layers] == ["PNAConv"] * 2 and not model.add_self_loop
    assert [(l.in_channels, l.out_channels) for l in model.gnn_layers] == [(dim, 64), (64, k)]
    op = pna_conv.agg_concat_pna
    if with_composite:
        pna_conv.agg_concat_pna = lambda h, rp, ci, names: composite(h, rp, ci, names)
    try:
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
    finally:
        pna_conv.agg_concat_pna = op
        wgth.destroy_wholememory_optimizer(wm_opt)
        wgth.destroy_embedding(emb)
        wgth.destroy_wholememory_tensor(wrow)
        wgth.destroy_wholememory_tensor(wcol)
    return losses, acc, changed, final


def test_two_layer_pna_model_trains_end_to_end_and_reproducibly(gpu_env):
    """The bars are those of the other end-to-end tests. The reference they were checked against: this model with
    agg_concat_pna replaced by the torch composite above (train_pna(..., with_composite=True)), on the MI355X, gave loss
    3.5013 -> 0.0028 (ratio 0.0008), accuracy 1.000 and every embedding row moved with seed 1 (the op itself: the same figures
    to four digits), ratio 0.038 / accuracy 0.987 with seed 2 and ratio 0.008 / accuracy 1.000 with seed 3: it clears
    `last < 0.6 * first` and accuracy > 0.7, so they stand."""
    import torch
    losses, acc, changed, final = train_pna(gpu_env, 1)
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print("loss %.3f -> %.3f, accuracy %.3f, changed %.3f" % (first, last, acc, changed))
    assert np.isfinite(losses).all()
    assert last < 0.6 * first, "loss %.3f -> %.3f" % (first, last)
    assert changed > 0.2, "gradients did not reach the WholeMemory embedding"
    assert acc > 0.7
    losses2, _, _, final2 = train_pna(gpu_env, 1)
    assert losses2 == losses
    assert torch.equal(final.view(torch.int32), final2.view(torch.int32))
