"""KGEModel (wholegraph_amd/torch/kge.py) on the MI355X: filtered negatives, the block of kge_block and kge_score_n2n on a
planted typed graph held in CHUNKED WholeMemory, the entity table in WholeMemory with the sparse SGD optimizer, the relation
table a dense parameter under torch's SGD.

The graph: 300 entities in 6 groups of 50 and 4 relations; relation k links a head of group i to a tail of group
(i + k) % 6; about 3000 distinct triples. F = 32, K = 4 negatives per triple, 30 steps over all triples at once.

The step sizes: the loss is a mean over about 3000 positive and 12000 negative edges and an entity is in about 70 of them, so
a row's gradient is about 70 / 3000 of a per-edge one; lr = 20 makes a step of about half a per-edge step of size 1. A
relation is in a quarter of all edges: lr = 1. The margins put the distance models' initial scores near 0."""
import numpy as np
import pytest

from test_kge_score_gpu import steps
from test_sage_agg_gpu import _wm_array

pytestmark = pytest.mark.gpu

N, GROUPS, R, DIM, K = 300, 6, 4, 32, 4
N_STEPS, LR, REL_LR = 30, 20.0, 1.0
MARGIN = {"distmult": 0.0, "complex": 0.0, "transe_l1": 3.0, "transe_l2": 1.0, "rotate": 1.0}
MODELS = list(MARGIN)
_GRAPH, _RUNS = {}, {}


def graph():
    """(row_ptr int64 [N + 1], col int64 [E] ascending per row, triples int64 [E, 3])"""
    if not _GRAPH:
        rng = np.random.default_rng(11)
        h = rng.integers(0, N, 3300)
        k = rng.integers(0, R, 3300)
        t = ((h // 50 + k) % GROUPS) * 50 + rng.integers(0, 50, 3300)
        _, first = np.unique(h * N + t, return_index=True)      # one relation per (head, tail): sorted by head, then tail
        h, k, t = h[first], k[first], t[first]
        row_ptr = np.zeros(N + 1, np.int64)
        np.cumsum(np.bincount(h, minlength=N), out=row_ptr[1:])
        _GRAPH["g"] = (row_ptr, t.astype(np.int64), np.stack([h, k, t], 1).astype(np.int64))
        assert 2900 < len(t) < 3300
    return _GRAPH["g"]


def setup(comm, name, seed):
    import torch
    import wholegraph_amd.torch as wgth
    row_ptr, col, _ = graph()
    wrow, wcol = _wm_array(comm, row_ptr), _wm_array(comm, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [N, DIM])
    torch.manual_seed(seed)
    emb.get_embedding_tensor().get_local_tensor()[0].copy_((torch.randn(N, DIM) * 0.1).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    model = wgth.KGEModel(g, emb, R, model=name, num_negatives=K, margin=MARGIN[name], col_sorted=True)
    torch.cuda.synchronize()
    return model, emb, (wm_opt, emb, wrow, wcol)


def teardown(things):
    import wholegraph_amd.torch as wgth
    for destroy, thing in zip((wgth.destroy_wholememory_optimizer, wgth.destroy_embedding) + (wgth.destroy_wholememory_tensor,) * 2,
                              things):
        destroy(thing)


def composite(self, x_src, x_dst, rel, batch):
    """KGEModel.score_edges in plain torch: three [E, F] gathers and the model's formula"""
    import torch
    deg = (batch.row_ptr[1:] - batch.row_ptr[:-1]).long()
    h = x_dst.index_select(0, torch.repeat_interleave(torch.arange(deg.numel(), device=x_src.device), deg))
    return steps(self.model, h, rel.index_select(0, batch.edge_type.long()), x_src.index_select(0, batch.col_ind.long()), None,
                 torch)


def train(comm, name, seed, fresh=False, score_edges=None):
    """N_STEPS steps over all triples -> (losses, entity table, relation parameter); cached per (model, seed, scorer)"""
    import torch
    key = (name, seed, score_edges is not None)
    if fresh or key not in _RUNS:
        model, emb, things = setup(comm, name, seed)
        if score_edges is not None:
            model.score_edges = score_edges.__get__(model)
        opt = torch.optim.SGD([model.relation], lr=REL_LR)
        triples = torch.from_numpy(graph()[2]).cuda()
        losses = []
        model.train()
        for step in range(N_STEPS):
            loss = model(triples, random_seed=1000 * seed + step)
            opt.zero_grad()
            loss.backward()
            things[0].step(LR)
            opt.step()
            losses.append(float(loss.detach()))
        _RUNS[key] = (losses, emb.get_embedding_tensor().get_local_tensor()[0].clone(), model.relation.detach().clone())
        teardown(things)
    return _RUNS[key]


def test_negatives_are_filtered_and_the_block_is_kge_block(gpu_env):
    import torch
    row_ptr, col, triples = graph()
    model, emb, things = setup(gpu_env, "distmult", 1)
    b = model.sample(torch.from_numpy(triples), random_seed=5)
    anchors, rp, ctx, ty, lab = (t.cpu().numpy() for t in (b.anchor_ids, b.row_ptr, b.ctx_ids, b.edge_type, b.labels))
    assert np.array_equal(anchors, triples[:, 0]) and rp.dtype == np.int32 and rp[-1] == len(ctx) == len(ty) == len(lab)
    assert np.array_equal(ctx[rp[:-1]], triples[:, 2]) and (lab[rp[:-1]] == 1).all() and lab.sum() == len(triples)
    assert np.array_equal(ty, np.repeat(triples[:, 1], np.diff(rp)))          # the relation repeated along the row
    deg = np.diff(rp)
    assert deg.max() == K + 1 and deg.min() >= 1 and deg.sum() > 0.9 * (K + 1) * len(triples)
    for c in np.random.default_rng(3).permutation(len(triples))[:600]:
        h = triples[c, 0]
        negs = ctx[rp[c] + 1:rp[c + 1]]
        assert not np.isin(negs, col[row_ptr[h]:row_ptr[h + 1]]).any() and (negs != h).all() and ((0 <= negs) & (negs < N)).all()
    uniq, ci = b.unique_ctx.cpu().numpy(), b.col_ind.cpu().numpy()
    assert len(np.unique(uniq)) == len(uniq) and np.array_equal(uniq[ci], ctx)
    teardown(things)


@pytest.mark.parametrize("name", MODELS)
def test_training_lowers_the_loss(gpu_env, name):
    losses = train(gpu_env, name, 1)[0]
    print("%s: loss %s" % (name, " ".join("%.4f" % v for v in losses)))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


@pytest.mark.parametrize("name", ["distmult", "rotate"])
def test_two_runs_end_with_the_same_bits_and_no_worse_than_the_composite(gpu_env, name):
    """The op's final loss may exceed the composite's with the same seed by at most the spread (max - min) of the composite's
    final loss over three seeds, measured in the same call. Measured on the MI355X (printed by the test, recorded in DESIGN.md
    section 3.25): distmult, the op 1.3872 -> 1.354654, the composite 1.354654 (seed 1), 1.3522 (2), 1.3519 (3), spread
    0.0027; rotate, the op 1.3997 -> 1.332661, the composite 1.332661 (1), 1.3338 (2), 1.3347 (3), spread 0.0020."""
    import torch
    losses, table, rel = train(gpu_env, name, 1)
    losses2, table2, rel2 = train(gpu_env, name, 1, fresh=True)
    assert losses2 == losses
    assert torch.equal(table.view(torch.int32), table2.view(torch.int32)) and torch.equal(rel.view(torch.int32), rel2.view(torch.int32))
    ref = {seed: train(gpu_env, name, seed, score_edges=composite)[0] for seed in (1, 2, 3)}
    for seed, curve in ref.items():
        print("%s, composite, seed %d: loss %s" % (name, seed, " ".join("%.4f" % v for v in curve)))
    finals = [c[-1] for c in ref.values()]
    spread = max(finals) - min(finals)
    print("%s: op final %.6f, composite final %.6f (seed 1), spread over three seeds %.6f" % (name, losses[-1], finals[0], spread))
    assert losses[-1] <= finals[0] + spread
