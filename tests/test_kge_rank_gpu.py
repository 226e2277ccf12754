"""KGEModel.rank / KGEModel.test (wholegraph_amd/torch/kge.py) on the MI355X against a float64 ranking in torch that scores
every entity with the model's own formula (header section 2u; the l2 models by the squared distance, which ranks alike).

300 entities, 3 relations, about 1500 distinct (head, tail) pairs, F = 16. Entity and relation rows are quarters in
[-0.5, 0.5] (rotate: unit relation entries 1, i, -1, -i), so every product and sum is exact in float32 and in float64 and
the two rankings agree exactly, ties included."""
import functools

import numpy as np
import pytest

from test_kge_model_gpu import teardown
from test_sage_agg_gpu import _wm_array

pytestmark = pytest.mark.gpu

N, R, DIM = 300, 3, 16
MODELS = ["distmult", "transe_l1", "transe_l2", "complex", "rotate"]


@functools.lru_cache(maxsize=None)
def graph():
    """(row_ptr int64 [N + 1], col int64 [E] ascending per row, triples int64 [E, 3])"""
    rng = np.random.default_rng(17)
    h, t = rng.integers(0, N, 1600), rng.integers(0, N, 1600)
    _, first = np.unique(h * N + t, return_index=True)
    h, t = h[first], t[first]
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(h, minlength=N))]).astype(np.int64)
    return row_ptr, t.astype(np.int64), np.stack([h, rng.integers(0, R, len(h)), t], 1).astype(np.int64)


def setup(comm, name, corrupt):
    """-> (model, entity table float32 [N, DIM] (cpu), relation rows float32 [R, DIM] (cpu), things to destroy)"""
    import torch
    import wholegraph_amd.torch as wgth
    row_ptr, col, _ = graph()
    wrow, wcol = _wm_array(comm, row_ptr), _wm_array(comm, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [N, DIM])
    rng = np.random.default_rng(23)
    table = torch.from_numpy(rng.integers(-2, 3, (N, DIM)).astype(np.float32) / 4)
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(table.cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    model = wgth.KGEModel(g, emb, R, model=name, num_negatives=2, corrupt=corrupt, col_sorted=True)
    if name == "rotate":
        turn = rng.integers(0, 4, (R, DIM // 2))
        rel = torch.from_numpy(np.concatenate([np.array([1, 0, -1, 0])[turn], np.array([0, 1, 0, -1])[turn]], 1).astype(np.float32))
        model.relation_rows = lambda: rel.cuda()
    else:
        rel = torch.from_numpy(rng.integers(-2, 3, (R, DIM)).astype(np.float32) / 4)
        with torch.no_grad():
            model.relation.copy_(rel.cuda())
    torch.cuda.synchronize()
    return model, table, rel, (wm_opt, emb, wrow, wcol)


def all_scores(name, h, r, t):
    """float64 [T, N]: h, r, t broadcast as [T, 1 or N, DIM]"""
    import torch
    if name == "distmult":
        return (h * r * t).sum(-1)
    if name.startswith("transe"):
        d = h + r - t
        return -d.abs().sum(-1) if name == "transe_l1" else -(d * d).sum(-1)
    c = lambda x: torch.complex(x[..., :DIM // 2], x[..., DIM // 2:])
    u, tc = c(h) * c(r), c(t)
    return (u * tc.conj()).real.sum(-1) if name == "complex" else -((u - tc).real ** 2 + (u - tc).imag ** 2).sum(-1)


def reference(name, corrupt, table, rel, triples, filtered):
    import torch
    row_ptr, col, _ = graph()
    e64 = table.double()
    anchor = e64[triples[:, 0 if corrupt == "tail" else 2]][:, None]
    r = rel.double()[triples[:, 1]][:, None]
    s = all_scores(name, anchor, r, e64[None]) if corrupt == "tail" else all_scores(name, e64[None], r, anchor)
    out = np.zeros((2, len(triples)), np.int64)
    for i, (h, _, t) in enumerate(triples):
        a, true = (h, t) if corrupt == "tail" else (t, h)
        keep = torch.ones(N, dtype=torch.bool)
        keep[true] = False
        if filtered:
            keep[col[row_ptr[a]:row_ptr[a + 1]]] = False
        out[0, i], out[1, i] = int((s[i][keep] > s[i, true]).sum()), int((s[i][keep] == s[i, true]).sum())
    return out


@pytest.mark.parametrize("corrupt", ["tail", "head"])
@pytest.mark.parametrize("name", MODELS)
def test_rank_equals_the_float64_ranking(gpu_env, name, corrupt):
    import torch
    triples = graph()[2][::7]
    model, table, rel, things = setup(gpu_env, name, corrupt)
    got = {}
    for filtered in (True, False):
        greater, equal = model.rank(torch.from_numpy(triples), filtered=filtered, batch_size=100)
        got[filtered] = np.stack([greater.cpu().numpy(), equal.cpu().numpy()])
        assert np.array_equal(got[filtered], reference(name, corrupt, table, rel, triples, filtered)), (name, corrupt, filtered)
    # the known neighbours are out of the filtered counts (the reference's keep mask) and were in the unfiltered ones
    assert (got[True] <= got[False]).all() and (got[True].sum(0) < got[False].sum(0)).any()
    teardown(things)


def test_metrics_follow_the_ranks(gpu_env):
    import torch
    triples = torch.from_numpy(graph()[2][::5])
    model, _, _, things = setup(gpu_env, "transe_l1", "tail")
    greater, equal = model.rank(triples)
    rank = 1.0 + greater.double().cpu().numpy() + equal.double().cpu().numpy() / 2
    mean_rank, mrr, hits = model.test(triples, k=(1, 3, 10))
    assert mean_rank == pytest.approx(rank.mean(), rel=1e-12) and mrr == pytest.approx((1 / rank).mean(), rel=1e-12)
    assert hits == {k: pytest.approx((rank <= k).mean(), rel=1e-12) for k in (1, 3, 10)}
    teardown(things)


def test_evaluation_leaves_training_alone(gpu_env):
    """a dozen steps end with the same table bits whether or not test() ran between them"""
    import torch
    triples = torch.from_numpy(graph()[2]).cuda()
    tables = []
    for evaluate in (False, True):
        model, _, _, things = setup(gpu_env, "distmult", "tail")
        opt = torch.optim.SGD([model.relation], lr=0.5)
        model.train()
        for step in range(12):
            loss = model(triples, random_seed=step)
            opt.zero_grad()
            loss.backward()
            things[0].step(5.0)
            opt.step()
            if evaluate and step % 4 == 1:
                model.test(triples[::9])
        tables.append(things[1].get_embedding_tensor().get_local_tensor()[0].clone())
        teardown(things)
    assert torch.equal(tables[0].view(torch.int32), tables[1].view(torch.int32))
