"""PinSAGE importance neighbourhoods on the MI355X (csrc/kernels/rwr.hip through GraphStructure) against tests/_rwr_ref.py, bit
for bit, `nodes` and `counts`: the ladder of tests/_walk_ref.py under six (R, L, restart_prob, T, seeds used) — one lane, a ragged
pass, a full wave, two passes, the largest table, rows of padding —, the star, a damaged col_ind, batch independence, the Python
layers up to PinSAGEModel. The references are computed once per case and shared."""
import types

import numpy as np
import pytest

import _rwr_ref
import _walk_ref as ref

pytestmark = pytest.mark.gpu

SEED = ref.LADDER_SEED
CASES = [(1, 1, 0.0, 1, 512), (7, 5, 0.0, 3, 512), (64, 4, 0.5, 10, 512), (65, 3, 0.15, 64, 256), (128, 16, 0.15, 64, 32),
         (16, 4, 0.9, 64, 512)]
_WANT = {}


def _damaged():      # the entries of test_damaged_col_ind_ends_walks: -1, n_nodes and 2^31 - 1 at every 7th position from 3
    bad = np.array(ref.ladder()[1])
    hit = np.arange(3, bad.shape[0], 7)
    bad[hit] = np.array([-1, ref.LADDER_NODES, (1 << 31) - 1], dtype=np.int64)[np.arange(hit.shape[0]) % 3]
    return bad


def _want(case, damaged=False):
    if (case, damaged) not in _WANT:
        row_ptr, col, _, starts = ref.ladder()
        R, L, p, T, m = case
        _WANT[case, damaged] = _rwr_ref.rwr_top(row_ptr, _damaged() if damaged else col, starts[:m], R, L, p, T, SEED)
    return _WANT[case, damaged]


def _graph(comm, mt, row_ptr, col):
    import wholegraph_amd.torch as wgth
    from test_c5_flow_gpu import _wm_array
    ts = [_wm_array(comm, mt, np.array(row_ptr), "cuda"), _wm_array(comm, mt, np.array(col), "cuda")]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    return g, lambda: [wgth.destroy_wholememory_tensor(t) for t in ts]


def _assert_equal(got, want, col_dtype, what):
    nodes, counts = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert nodes.dtype == col_dtype and counts.dtype == np.int32, what
    assert np.array_equal(nodes, want[0].astype(col_dtype)) and np.array_equal(counts, want[1]), "nodes or counts differ: %s" % (what,)


@pytest.mark.parametrize("mt", ["continuous", "chunked"])
@pytest.mark.parametrize("col_dtype,seed_dtype", [(np.int32, np.int64), (np.int64, np.int32)])
@pytest.mark.parametrize("k", range(len(CASES)))
def test_ladder_equals_the_reference(gpu_env, k, col_dtype, seed_dtype, mt):
    import torch
    R, L, p, T, m = CASES[k]
    want = _want(CASES[k])
    met = want[2]
    # the reference alone: every case stays populated (half of what the unchanged ladder gives)
    assert met["tie_at_cut"] >= {1: 100, 2: 100, 4: 12}.get(k, 0) and met["maxdistinct"] >= (450 if k == 4 else 0), met
    assert met["short"] >= (250 if k == 5 else 0) and (k == 0 or met["dead"] >= 100), met
    row_ptr, col, _, starts = ref.ladder()
    outside = (starts[:m] < 0) | (starts[:m] >= ref.LADDER_NODES)      # three seeds outside the graph: all-padding rows
    assert (m < 512 or outside.sum() == 3) and (want[0][outside] == -1).all() and (want[1][outside] == 0).all()
    g, done = _graph(gpu_env, mt, row_ptr, col.astype(col_dtype))
    seeds = torch.from_numpy(starts[:m].astype(seed_dtype)).cuda()
    got = g.pinsage_neighbors(seeds, T, num_walks=R, walk_length=L, restart_prob=p, random_seed=SEED)
    _assert_equal(got, want, col_dtype, CASES[k])
    done()


def test_star_and_damaged_col_ind_equal_the_reference(gpu_env):
    """star: from the centre the eight leaves tie often, from a leaf every second arrival is the seed itself and is dropped.
    damaged col_ind: the range check is all that stands between a bad id and row_ptr; every id written is a node or -1"""
    import torch
    row_ptr, col, _ = ref.star()
    seeds = np.array([0, 3], dtype=np.int64)
    g, done = _graph(gpu_env, "continuous", row_ptr, col)
    for T in (4, 64):
        want = _rwr_ref.rwr_top(row_ptr, col, seeds, 64, 4, 0.5, T, ref.STAR_SEED)
        assert want[0][1, 0] == 0 and 3 not in want[0][1] and (want[0][0, :min(T, 8)] > 0).all() and (want[0][0, 8:] < 0).all()
        got = g.pinsage_neighbors(torch.from_numpy(seeds).cuda(), T, num_walks=64, walk_length=4, restart_prob=0.5, random_seed=ref.STAR_SEED)
        _assert_equal(got, want, np.int64, "star, T = %d" % T)
    done()
    R, L, p, T, m = CASES[2]
    want = _want(CASES[2], damaged=True)
    assert want[2]["dead"] >= _want(CASES[2])[2]["dead"] + 100, "too few walkers meet a damaged entry"
    g, done = _graph(gpu_env, "chunked", ref.ladder()[0], _damaged().astype(np.int32))
    got = g.pinsage_neighbors(torch.from_numpy(np.array(ref.ladder()[3])).cuda(), T, num_walks=R, walk_length=L, restart_prob=p, random_seed=SEED)
    _assert_equal(got, want, np.int32, "damaged")
    assert ((got[0] >= -1) & (got[0] < ref.LADDER_NODES)).all()
    done()


def test_batch_independence_the_same_seed_twice_the_empty_batch_and_distributed(gpu_env):
    import torch
    from wholegraph_amd import binding
    row_ptr, col, _, starts = ref.ladder()
    g, done = _graph(gpu_env, "chunked", row_ptr, col)
    seeds = torch.from_numpy(np.array(starts)).cuda()
    kw = dict(num_walks=64, walk_length=4, restart_prob=0.5, random_seed=SEED)
    whole, again, first = g.pinsage_neighbors(seeds, 10, **kw), g.pinsage_neighbors(seeds, 10, **kw), g.pinsage_neighbors(seeds[:100], 10, **kw)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)), "the same seed, another result"
    assert all(torch.equal(a[:100], b) for a, b in zip(whole, first)), "a row depends on its batch"
    nodes, counts = g.pinsage_neighbors(seeds[:0], 7, **kw)
    assert tuple(nodes.shape) == (0, 7) and tuple(counts.shape) == (0, 7) and nodes.dtype == torch.int64
    done()
    g, done = _graph(gpu_env, "distributed", row_ptr, col)      # (such a tensor needs a device: pinned here, not in the surface test)
    with pytest.raises(binding.WholeMemoryError) as e:
        g.pinsage_neighbors(seeds, 10, **kw)
    assert e.value.code == 2 and isinstance(e.value, NotImplementedError)      # WHOLEMEMORY_NOT_IMPLEMENTED
    done()


def test_python_layers_up_to_the_model(gpu_env):
    import torch
    import torch.nn.functional as F
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import weighted_aggregation as wa
    row_ptr, col, _, starts = ref.ladder()
    g, done = _graph(gpu_env, "chunked", row_ptr, col)
    seeds = torch.from_numpy(np.array(starts)).cuda()
    kw = dict(num_walks=16, walk_length=4, restart_prob=0.5)
    nodes, counts = g.pinsage_neighbors(seeds, 5, random_seed=11, **kw)
    offsets, neigh, lid, imp = g.pinsage_sample_one_hop(seeds, 5, random_seed=11, need_center_local_output=True, **kw)
    kept = nodes >= 0
    assert torch.equal(neigh, nodes[kept]) and torch.equal(lid.long(), torch.nonzero(kept)[:, 0]) and offsets.dtype == torch.int32
    assert torch.equal(offsets.long(), F.pad(kept.sum(1).cumsum(0), (1, 0))) and imp.dtype == torch.float32
    sums = torch.zeros(512, device="cuda").index_add_(0, lid.long(), imp)
    # at most 64 fp32 terms in (0, 1], each rounded once, summed with 63 roundings of sums below 2: (64 + 63) half-ulps of 2
    assert ((sums - (kept.sum(1) > 0).float()).abs() <= 127 * 2.0 ** -24).all() and (kept.sum(1) == 0).sum() >= 3
    batch = seeds[(seeds >= 0) & (seeds < ref.LADDER_NODES)]
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [ref.LADDER_NODES, 32])
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(torch.randn(ref.LADDER_NODES, 32, generator=torch.Generator().manual_seed(3)).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    wgth.set_framework("cugraph")
    model = wgth.PinSAGEModel(g, emb, types.SimpleNamespace(hiddensize=64, layernum=2, classnum=5, dropout=0.0, neighbors="5,5", **kw)).cuda()
    gids, _, row_ptrs, col_inds, imps = model.sample(batch, [21, 22])
    assert len(gids) == 3 and torch.equal(gids[-1], batch) and all(w.shape == c.shape for w, c in zip(imps, col_inds))
    log = list(wa.backward_requests)      # (a bounded log that tests/test_weighted_agg_gpu.py counts: left as it was found)
    logits = model(batch, random_seeds=[21, 22])
    F.cross_entropy(logits, (batch % 5).long()).backward()
    assert tuple(logits.shape) == (batch.shape[0], 5) and torch.isfinite(logits).all() and len(emb.sparse_grads) == 1
    assert all(torch.isfinite(p.grad).all() and (p.grad != 0).any() for p in model.parameters() if p.requires_grad)
    wa.backward_requests[:] = log
    # layer 0's aggregation against float64 torch. tests/test_weighted_agg_gpu.py compares this op bit for bit with the sum of
    # fl(w * x) taken left to right in fp32; a float64 product or sum of two fp32 values rounded to fp32 IS the fp32 operation
    # (53 >= 2 * 24 + 2), so the same zero tolerance holds here
    x = emb.gather(gids[0]).float()
    off, ci, w = row_ptrs[0].long(), col_inds[0].long(), imps[0]
    want = torch.zeros(off.shape[0] - 1, 32, device="cuda")
    for j in range(5):
        rows = torch.nonzero(off[1:] - off[:-1] > j)[:, 0]
        term = (w[off[rows] + j].double()[:, None] * x[ci[off[rows] + j]].double()).float()
        want[rows] = (want[rows].double() + term.double()).float()
    got = wa.agg_concat_weighted(x, row_ptrs[0], col_inds[0], w, "sum")
    assert torch.equal(got[:, :32], want) and torch.equal(got[:, 32:], x[:want.shape[0]]) and (want != 0).any()
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    done()
