"""topk_rows (header section 2x) and KGEModel.predict on the MI355X against the contract restated in numpy: test_rank_gpu's
float32 accumulator column by column, then a sort by (-score, id) with -0.0 folded into +0.0, NaN rows and the filter row
dropped, the first k taken and the tail -1 / NaN. Ids and scores are compared exactly.

The sweep's tile is 256 rows x 64 queries: N = 769 is three row tiles and one row (four tiles: the table is split among
workgroups whose partial tops are merged), B = 65 and 63 one more and one fewer than a query tile; the F are test_rank_gpu's."""
import functools

import numpy as np
import pytest

from test_rank_gpu import F32, MEASURES, N, case, scores

pytestmark = pytest.mark.gpu


def top(s, k, begin=0, end=None, filt=None):
    """(ids int64 [B, k], scores float32 [B, k]) from a score matrix s of any float type"""
    ids, val = np.full((s.shape[0], k), -1, np.int64), np.full((s.shape[0], k), np.nan, F32)
    for b in range(s.shape[0]):
        keep = np.zeros(s.shape[1], bool)
        keep[begin:end] = True
        if filt is not None:
            f = np.asarray(filt[b], np.int64)
            keep[f[(f >= 0) & (f < s.shape[1])]] = False
        rows = np.flatnonzero(keep & ~np.isnan(s[b]))
        v = s[b, rows] + 0.0      # (-0.0 + 0.0 is +0.0)
        best = rows[np.lexsort((rows, -v))][:k]
        ids[b, :len(best)], val[b, :len(best)] = best, s[b, best] + 0.0
    return ids, val


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)


def run(comm, table, query, k, measure, filt=None, entity_range=None, id_dtype=np.int64, mt="continuous", pad=0):
    """the op over `table` as a WholeMemory tensor, or (pad > 0) as the view [1:, 1 : 1 + F] of one with a row and `pad` columns more"""
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
        row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in filt])]).astype(np.int32 if id_dtype == np.int32 else np.int64)
        ids = np.concatenate([np.asarray(r, id_dtype) for r in filt] + [np.zeros(0, id_dtype)])
        kw = dict(filter_row_ptr=torch.from_numpy(row_ptr).cuda(), filter_ids=torch.from_numpy(ids).cuda())
    ids, val = wholegraph_ops.topk_rows(owner.get_sub_tensor([1, 1], [n + 1, 1 + f]) if pad else owner, torch.from_numpy(query).cuda(),
                                        k, measure=measure, entity_range=entity_range, **kw)
    out = ids.cpu().numpy(), val.cpu().numpy()
    wgth.destroy_wholememory_tensor(owner)
    return out


def mixed_filter(seed, s):
    """per query, ascending: empty every fourth, else every third of the best 40 rows (one of them twice), five others and ids
    outside the table"""
    rng = np.random.default_rng(seed)
    return [[] if b % 4 == 0 else np.sort(np.concatenate([np.argsort(-s[b], kind="stable")[:40:3], np.argsort(-s[b])[:1],
                                                          rng.integers(0, s.shape[1], 5), [-1, s.shape[1], s.shape[1] + 5]]))
            for b in range(s.shape[0])]


@functools.lru_cache(maxsize=None)
def contract_case(f, b, measure):
    table, query, _ = case(f, b)
    s = scores(table, query, measure)
    return table, query, s, mixed_filter(f, s)


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("f,b", [(1, 65), (3, 63), (33, 65), (128, 63), (200, 65)])
def test_top_follows_the_contract(gpu_env, measure, f, b, k):
    table, query, s, filt = contract_case(f, b, measure)
    want = top(s, k, filt=filt)
    assert not same(want, top(s, k))      # (the filter changes the answer)
    assert same(run(gpu_env, table, query, k, measure, filt), want)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
def test_ties_on_dyadic_rows_and_the_filter(gpu_env, measure, id_dtype):
    table, query, _ = case(12, 65, 5, dyadic=True)
    s, t64, q64 = scores(table, query, measure), table.astype(np.float64), query.astype(np.float64)
    exact = {"dot": q64 @ t64.T, "l1": -np.abs(q64[:, None] - t64[None]).sum(2), "l2": -((q64[:, None] - t64[None]) ** 2).sum(2)}[measure]
    want = top(s, 64)
    assert (want[1][:, 0] == want[1][:, 5]).any() and np.array_equal(want[0], top(exact, 64)[0])
    assert same(run(gpu_env, table, query, 64, measure), want)
    filt = mixed_filter(9, s)
    assert same(run(gpu_env, table, query, 64, measure, filt, id_dtype=id_dtype), top(s, 64, filt=filt))


@pytest.mark.parametrize("measure", MEASURES)
def test_short_answers(gpu_env, measure):
    """fewer than k rows: a range of 5, an empty range, a filter that leaves 3 rows, and a table row of NaN that is never returned"""
    table, query, _ = case(33, 65)
    table = table.copy()
    table[2] = np.nan
    s = scores(table, query, measure)
    for r in ((300, 305), (0, 5), (7, 7)):
        got = run(gpu_env, table, query, 10, measure, entity_range=r)
        assert same(got, top(s, 10, *r)) and (got[0][:, 5:] == -1).all() and np.isnan(got[1][:, 5:]).all() and (got[0] != 2).all()
    filt = [np.delete(np.arange(N), [2, 5 + b, 400, 768]) for b in range(65)]
    got = run(gpu_env, table, query, 10, measure, filt)
    assert same(got, top(s, 10, filt=filt)) and (got[0][:, 3:] == -1).all() and (got[0][:, :3] >= 0).all()
    got = run(gpu_env, table, query[:0], 10, measure)
    assert got[0].shape == (0, 10) and got[1].shape == (0, 10)


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("mt,pad,f", [("continuous", 0, 33), ("chunked", 0, 128), ("continuous", 7, 128), ("chunked", 3, 33)])
def test_disjoint_ranges_merge_to_the_whole(gpu_env, measure, mt, pad, f):
    """also a single-rank CHUNKED table and views with a storage offset and a padded row stride (element-wise loads)"""
    table, query, _ = case(f, 63, 8)
    s = scores(table, query, measure)
    pieces = []
    for r in ((0, 100), (100, 613), (613, N)):
        pieces.append(run(gpu_env, table, query, 10, measure, entity_range=r, mt=mt, pad=pad))
        assert same(pieces[-1], top(s, 10, *r))
    ids, val = np.concatenate([p[0] for p in pieces], 1), np.concatenate([p[1] for p in pieces], 1)
    order = np.stack([np.lexsort((ids[b], -val[b]))[:10] for b in range(63)])
    merged = np.take_along_axis(ids, order, 1), np.take_along_axis(val, order, 1)
    assert same(merged, top(s, 10)) and same(run(gpu_env, table, query, 10, measure, mt=mt, pad=pad), merged)


@pytest.mark.parametrize("cap", [1, 3])
def test_capped_grid(gpu_env, knobs, cap):
    """4 query tiles x 4 row splits under WM_AGG_MAX_BLOCKS: one workgroup walks every (query tile, split) pair"""
    table, query, _ = case(12, 200, 5, dyadic=True)
    s = scores(table, query, "l1")
    filt = mixed_filter(2, s)
    free = run(gpu_env, table, query, 64, "l1", filt)
    knobs.set("WM_AGG_MAX_BLOCKS", str(cap))
    assert same(run(gpu_env, table, query, 64, "l1", filt), free) and same(free, top(s, 64, filt=filt))


def test_positions_agree_with_rank_rows(gpu_env):
    """for every returned (b, j, e): rank_rows with target e and the same filter has greater <= j <= greater + equal"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import wholegraph_ops
    table, query, _ = case(12, 65, 5, dyadic=True)
    filt = [np.unique(r) for r in mixed_filter(4, scores(table, query, "l2"))]
    owner = wgth.create_wholememory_tensor(gpu_env, "continuous", "cuda", list(table.shape), torch.float32, None)
    owner.get_local_tensor()[0].copy_(torch.from_numpy(table))
    kw = dict(measure="l2", filter_row_ptr=torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in filt])])).cuda(),
              filter_ids=torch.from_numpy(np.concatenate(filt).astype(np.int64)).cuda())
    q = torch.from_numpy(query).cuda()
    ids, _ = wholegraph_ops.topk_rows(owner, q, 10, **kw)
    assert (ids >= 0).all()
    for j in range(10):
        greater, equal = wholegraph_ops.rank_rows(owner, q, ids[:, j].contiguous(), **kw)
        assert ((greater <= j) & (j <= greater + equal)).all(), j
    wgth.destroy_wholememory_tensor(owner)


@pytest.mark.parametrize("corrupt", ["tail", "head"])
@pytest.mark.parametrize("name", ["distmult", "transe_l2"])
def test_predict_equals_the_top_of_the_query_scores(gpu_env, name, corrupt):
    import torch
    from test_kge_model_gpu import teardown
    from test_kge_rank_gpu import graph, setup
    row_ptr, col, triples = graph()
    triples = triples[::7]
    model, table, rel, things = setup(gpu_env, name, corrupt)
    anchors, rels = triples[:, 0 if corrupt == "tail" else 2], triples[:, 1]
    before = things[1].get_embedding_tensor().get_local_tensor()[0].clone()
    got = model.predict(torch.from_numpy(anchors), torch.from_numpy(rels), 10, batch_size=100)
    query = model.rank_queries(table[anchors].cuda(), rel[rels].cuda()).cpu().numpy()
    s = scores(table.numpy(), query, "dot" if name == "distmult" else "l2")
    want = top(s, 10, filt=[col[row_ptr[a]:row_ptr[a + 1]] for a in anchors])
    assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want) and not same(want, top(s, 10))
    assert torch.equal(before, things[1].get_embedding_tensor().get_local_tensor()[0])
    teardown(things)
