"""rank_rows (header section 2w) on the MI355X against the contract restated in numpy: one float32 accumulator per (query, row)
over ascending columns, every operation rounded on its own (numpy rounds each float32 operation), then > and == against the
target's own value, the target and the filter row taken out. Counts are compared exactly.

The sweep's tile is 256 rows x 64 queries x 32 columns. N = 769 is three row tiles and one row, B = 65 and 63 one more and one
fewer than a query tile; F = 1, 3 and 33 take the element-wise loads and pad the last slice, 128 is four whole slices of
16-byte loads, 200 six slices and a quarter."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, N, MEASURES = np.float32, 769, ["dot", "l1", "l2"]


def scores(table, query, measure):
    """[B, N] float32: the contract's accumulator, column by column"""
    acc = np.zeros((query.shape[0], table.shape[0]), F32)
    for c in range(table.shape[1]):
        u, t = query[:, c:c + 1], table[None, :, c]
        acc = acc + (u * t if measure == "dot" else np.abs(u - t) if measure == "l1" else (u - t) * (u - t))
    return acc if measure == "dot" else -acc


def counts(s, target, begin=0, end=N, filt=None):
    """(greater, equal) int64 [B] from a score matrix s of any float type; filt: a list of id arrays, one per query"""
    out = np.full((2, s.shape[0]), -1, np.int64)
    for b, t in enumerate(target):
        if 0 <= t < N:
            keep = np.zeros(N, bool)
            keep[begin:end] = True
            keep[t] = False
            if filt is not None:
                ids = np.asarray(filt[b], np.int64)
                keep[ids[(ids >= 0) & (ids < N)]] = False
            out[:, b] = (s[b, keep] > s[b, t]).sum(), (s[b, keep] == s[b, t]).sum()
    return out


def run(comm, table, query, target, measure, filt=None, entity_range=None, id_dtype=np.int64, mt="continuous", pad=0):
    """the op over `table` as a WholeMemory tensor, or (pad > 0) as the view [1:, 1 : 1 + F] of one with a row and `pad`
    columns more: a storage offset and a row stride of F + pad"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import wholegraph_ops
    n, f = table.shape
    full = np.full((n + 1, f + pad), 7.0, F32) if pad else table
    if pad:
        full[1:, 1:1 + f] = table
    owner = wgth.create_wholememory_tensor(comm, mt, "cuda", list(full.shape), torch.float32, None)
    owner.get_local_tensor()[0].copy_(torch.from_numpy(full))
    kw = {}
    if filt is not None:
        row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in filt])]).astype(np.int64)
        ids = np.concatenate([np.asarray(r, id_dtype) for r in filt])
        kw = dict(filter_row_ptr=torch.from_numpy(row_ptr).cuda(), filter_ids=torch.from_numpy(ids).cuda())
    g, e = wholegraph_ops.rank_rows(owner.get_sub_tensor([1, 1], [n + 1, 1 + f]) if pad else owner, torch.from_numpy(query).cuda(),
                                    torch.from_numpy(target.astype(id_dtype)).cuda(), measure=measure, entity_range=entity_range, **kw)
    out = np.stack([g.cpu().numpy(), e.cpu().numpy()])
    wgth.destroy_wholememory_tensor(owner)
    return out


def case(f, b, seed=3, dyadic=False):
    """(table [N, f], query [b, f], target [b]). dyadic: quarters in [-0.5, 0.5], the table's rows drawn from 24 distinct ones:
    every order of the sum is exact and ties abound"""
    rng = np.random.default_rng(seed)
    if dyadic:
        return (rng.integers(-2, 3, (24, f)).astype(F32) / 4)[rng.integers(0, 24, N)], rng.integers(-2, 3, (b, f)).astype(F32) / 4, rng.integers(0, N, b)
    return rng.standard_normal((N, f)).astype(F32), rng.standard_normal((b, f)).astype(F32), rng.integers(0, N, b)


def mixed_filter(seed, s, target):
    """per query: empty every fourth, else the target, ids outside the table and distinct rows above, at and below the threshold"""
    rng, filt = np.random.default_rng(seed), []
    for b, t in enumerate(target):
        others = np.arange(N) != t
        picks = [rng.permutation(np.flatnonzero(m & others))[:5] for m in (s[b] > s[b, t], s[b] == s[b, t], s[b] < s[b, t])]
        filt.append([] if b % 4 == 0 else rng.permutation(np.concatenate(picks + [[t, -1, N, N + 5]])))
    return filt


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("f,b", [(1, 65), (3, 63), (33, 65), (128, 63), (200, 65)])
def test_counts_follow_the_contract(gpu_env, measure, f, b):
    table, query, target = case(f, b)
    s = scores(table, query, measure)
    filt = mixed_filter(f, s, target)
    assert np.array_equal(run(gpu_env, table, query, target, measure, filt), counts(s, target, filt=filt))


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
def test_ties_on_dyadic_rows_and_the_filter(gpu_env, measure, id_dtype):
    table, query, target = case(12, 65, 5, dyadic=True)
    s, t64, q64 = scores(table, query, measure), table.astype(np.float64), query.astype(np.float64)
    exact = {"dot": q64 @ t64.T, "l1": -np.abs(q64[:, None] - t64[None]).sum(2), "l2": -((q64[:, None] - t64[None]) ** 2).sum(2)}[measure]
    want = counts(s, target)
    assert want[1].min() > 5 and np.array_equal(want, counts(exact, target))
    assert np.array_equal(run(gpu_env, table, query, target, measure, id_dtype=id_dtype), want)
    filt = mixed_filter(9, s, target)
    assert np.array_equal(run(gpu_env, table, query, target, measure, filt, id_dtype=id_dtype), counts(s, target, filt=filt))


@pytest.mark.parametrize("measure", MEASURES)
def test_ranges_add_up_and_edge_cases(gpu_env, measure):
    table, query, target = case(33, 65)
    target[:3] = [-1, N, 700]                       # two outside the table; 700 lies outside the first two pieces
    s = scores(table, query, measure)
    whole, pieces = counts(s, target), []
    assert (whole[:, :2] == -1).all()
    for r in ((0, 100), (100, 613), (613, N)):
        pieces.append(run(gpu_env, table, query, target, measure, entity_range=r))
        assert np.array_equal(pieces[-1], counts(s, target, *r))
    assert np.array_equal(sum(p[:, 2:] for p in pieces), whole[:, 2:])
    empty = run(gpu_env, table, query, target, measure, entity_range=(5, 5))
    assert (empty[:, :2] == -1).all() and (empty[:, 2:] == 0).all()
    assert run(gpu_env, table, query[:0], target[:0], measure).shape == (2, 0)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("mt,pad,f", [("chunked", 0, 128), ("chunked", 3, 33), ("continuous", 7, 128), ("continuous", 4, 64)])
def test_chunked_tables_and_padded_views(gpu_env, measure, mt, pad, f):
    """a single-rank CHUNKED table, and views with a storage offset and a padded row stride (both element-wise loads)"""
    table, query, target = case(f, 63, 8)
    assert np.array_equal(run(gpu_env, table, query, target, measure, mt=mt, pad=pad), counts(scores(table, query, measure), target))


@pytest.mark.parametrize("cap", [1, 3])
def test_capped_grid(gpu_env, knobs, cap):
    """16 (row tile, query tile) pairs and a filter of about two thousand entries under WM_AGG_MAX_BLOCKS: later trips of every loop"""
    table, query, target = case(12, 200, 5, dyadic=True)
    s = scores(table, query, "l1")
    filt = mixed_filter(2, s, target)
    knobs.set("WM_AGG_MAX_BLOCKS", str(cap))
    assert np.array_equal(run(gpu_env, table, query, target, "l1", filt), counts(s, target, filt=filt))
