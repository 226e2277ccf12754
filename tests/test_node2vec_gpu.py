"""Node2Vec (wholegraph_amd/torch/node2vec.py) on the MI355X: walks, negatives, the skip-gram block and edge_dot_n2n on a
planted-partition graph held in CHUNKED WholeMemory, the embedding table in WholeMemory with the sparse SGD optimizer.

What a batch holds; two runs from the same seeds end with bit-identical tables; training lowers the loss and pulls the
communities apart; and the same run with edge_dot_n2n replaced by the torch composite is the reference for quality.

The step size: the loss is a mean over about 1.2e5 positive and 6.6e4 negative edges, so a row's gradient is about
1e-4 of what per-edge skip-gram updates (step 0.025) would add up to; lr = 2000 puts a step of the full batch there."""
import numpy as np
import pytest

from test_sage_agg_gpu import _planted_partition, _wm_array

pytestmark = pytest.mark.gpu

F32 = np.float32
N, K_COMM, DIM = 2000, 4, 32
WALK, WINDOW, NEG = 10, 3, 3
STEPS, LR = 20, 2000.0
_GRAPH = {}


def graph():
    if not _GRAPH:
        _GRAPH["g"] = _planted_partition(N, K_COMM, np.random.default_rng(2))
    return _GRAPH["g"]


def setup(comm, seed, **kw):
    """(model, embedding, things to destroy) with the table initialised from `seed`"""
    import torch
    import wholegraph_amd.torch as wgth
    row_ptr, col, _ = graph()
    wrow, wcol = _wm_array(comm, row_ptr), _wm_array(comm, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [N, DIM])
    init = torch.randn(N, DIM, generator=torch.Generator().manual_seed(seed)) * 0.1
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(init.cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    torch.cuda.synchronize()
    model = wgth.Node2Vec(g, emb, walk_length=WALK, window=WINDOW, num_negatives=NEG, col_sorted=True, **kw)
    return model, emb, (wm_opt, emb, wrow, wcol)


def teardown(things):
    import wholegraph_amd.torch as wgth
    wm_opt, emb, wrow, wcol = things
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


def table_of(emb):
    return emb.get_embedding_tensor().get_local_tensor()[0].clone()


def accuracy(table):
    """nearest-centroid community accuracy of the rows"""
    labels = graph()[2]
    x = table.cpu().numpy().astype(np.float64)
    cent = np.stack([x[labels == c].mean(0) for c in range(K_COMM)])
    return float((((x[:, None, :] - cent[None]) ** 2).sum(-1).argmin(1) == labels).mean())


def train(comm, seed, **kw):
    """STEPS steps from every node; -> (losses, final table)"""
    import torch
    model, emb, things = setup(comm, seed, **kw)
    starts = torch.arange(N, dtype=torch.int64, device="cuda")
    losses = []
    model.train()
    for step in range(STEPS):
        loss = model(starts, random_seed=1000 * seed + step)
        loss.backward()
        things[0].step(LR)
        losses.append(float(loss.detach()))
    table = table_of(emb)
    teardown(things)
    return losses, table


def composite(x_src, x_dst, row_ptr, col_ind):
    import torch
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(deg.numel(), device=x_src.device), deg)
    return (x_dst.index_select(0, dst) * x_src.index_select(0, col_ind.long())).sum(-1)


@pytest.mark.parametrize("p,q", [(1.0, 1.0), (0.5, 2.0)])
def test_sample_shape_and_contents(gpu_env, p, q):
    import torch
    row_ptr, col, _ = graph()
    model, emb, things = setup(gpu_env, 1, p=p, q=q)
    starts = torch.from_numpy(np.random.default_rng(5).permutation(N)[:64].astype(np.int64)).cuda()
    b = model.sample(starts, random_seed=77)
    walks = b.walks.cpu().numpy()
    assert walks.shape == (64, WALK + 1) and np.array_equal(walks[:, 0], starts.cpu().numpy())
    centres, rp, ctx, lab = (t.cpu().numpy() for t in (b.center_ids, b.row_ptr, b.ctx_ids, b.labels))
    assert np.array_equal(centres, walks[walks >= 0])            # every centre is a walk node, in row-major order
    assert rp.dtype == np.int32 and rp[0] == 0 and rp[-1] == len(ctx) == len(lab) and len(rp) == len(centres) + 1
    where = np.argwhere(walks >= 0)
    n_pos = n_neg = 0
    for c, (i, t) in enumerate(where):
        e0, e1 = rp[c], rp[c + 1]
        k = int(lab[e0:e1].sum())
        assert (lab[e0:e0 + k] == 1).all() and (lab[e0 + k:e1] == 0).all()   # positives first
        near = [walks[i, t + d] for d in list(range(-WINDOW, 0)) + list(range(1, WINDOW + 1))
                if 0 <= t + d <= WALK and walks[i, t + d] >= 0]
        assert ctx[e0:e0 + k].tolist() == near                   # within `window` of the centre on the same walk
        nbrs = set(col[row_ptr[centres[c]]:row_ptr[centres[c] + 1]].tolist())
        for v in ctx[e0 + k:e1]:
            assert v != centres[c] and v not in nbrs and 0 <= v < N   # no negative is the centre or a neighbour of it
        assert e1 - e0 - k <= NEG
        n_pos, n_neg = n_pos + k, n_neg + e1 - e0 - k
    assert n_pos > 0 and n_neg > 0.9 * NEG * len(centres)
    uniq, ci = b.unique_ctx.cpu().numpy(), b.col_ind.cpu().numpy()
    assert ci.dtype == np.int32 and len(np.unique(uniq)) == len(uniq) and (uniq >= 0).all()
    assert np.array_equal(uniq[ci], ctx)                         # col_ind maps back to ctx_ids
    loss = model.loss(b)
    assert loss.dim() == 0 and abs(float(loss.detach()) - 2 * np.log(2)) < 0.1   # scores near 0 on the small initial rows
    ids = torch.tensor([3, 1999, 3], device="cuda")
    assert torch.equal(model.embed(ids), table_of(emb)[ids])
    teardown(things)


def test_trains_reproducibly_and_as_well_as_the_composite(gpu_env, monkeypatch):
    """The op's run may fall short of the composite's accuracy with the same seed by at most the spread (max - min) of the
    composite's accuracy over three seeds, measured in the same call; the composite itself must be above chance, 1 / 4.
    Measured on the MI355X (printed by the test, recorded in DESIGN.md section 3.20): the op, seed 1, loss 1.3871 -> 1.0660
    and accuracy 0.3105 -> 1.0000; the composite loss 1.3871 -> 1.0660 (seed 1), 1.3870 -> 1.0629 (2), 1.3872 -> 1.0620 (3),
    accuracy 1.0000 each, spread 0."""
    import torch
    from wholegraph_amd.torch import node2vec
    labels = graph()[2]
    before = accuracy(torch.randn(N, DIM, generator=torch.Generator().manual_seed(1)) * 0.1)
    losses, table = train(gpu_env, 1)
    losses2, table2 = train(gpu_env, 1)
    assert losses2 == losses and torch.equal(table.view(torch.int32), table2.view(torch.int32))   # bit-identical tables
    assert np.isfinite(losses).all() and bool(torch.isfinite(table).all())
    acc = accuracy(table)
    print("edge_dot_n2n: loss %.4f -> %.4f, accuracy %.4f -> %.4f" % (losses[0], losses[-1], before, acc))
    assert losses[-1] < losses[0]
    x = table.double()
    rng = np.random.default_rng(9)
    a, b = (torch.from_numpy(rng.integers(0, N, 20000)).cuda() for _ in range(2))
    same = torch.from_numpy(labels[a.cpu().numpy()] == labels[b.cpu().numpy()]).cuda() & (a != b)
    s = (x[a] * x[b]).sum(-1)
    print("mean score: same community %.4f, across %.4f" % (float(s[same].mean()), float(s[~same & (a != b)].mean())))
    assert float(s[same].mean()) > float(s[~same & (a != b)].mean())
    monkeypatch.setattr(node2vec, "edge_dot_n2n", composite)
    ref = {}
    for seed in (1, 2, 3):
        ref_losses, ref_table = train(gpu_env, seed)
        ref[seed] = (ref_losses[-1], accuracy(ref_table))
        print("composite, seed %d: loss %.4f -> %.4f, accuracy %.4f" % (seed, ref_losses[0], ref_losses[-1], ref[seed][1]))
    accs = [v[1] for v in ref.values()]
    spread = max(accs) - min(accs)
    print("composite accuracy spread over three seeds: %.4f" % spread)
    assert min(accs) > 1.0 / K_COMM, "the composite does not beat chance: more steps are needed"
    assert acc >= ref[1][1] - spread, "accuracy %.4f, composite %.4f, spread %.4f" % (acc, ref[1][1], spread)
