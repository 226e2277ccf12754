"""Subgraph-wise training on the MI355X: GraphStructure.saint_random_walk_subgraph (walks, the sorted distinct nodes they visit,
the subgraph those induce) against the composition of the Python restatements of its pieces (tests/_walk_ref.py,
tests/_isub_ref.py), bit for bit, and SubgraphGNNModel (wholegraph_amd/torch/saint.py) against its own layers called by hand
on the reference block: the same ops in the same order, so the comparison is exact."""
import types

import numpy as np
import pytest

import _isub_ref as isub_ref
import _walk_ref as walk_ref

pytestmark = pytest.mark.gpu

STEPS, SEED = 4, 20240607
N, DIM, CLASSES = walk_ref.LADDER_NODES, 32, 5
_CACHE = {}


def _wm_array(comm, mt, arr):
    from test_c5_flow_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr))


def _destroy(ts):
    import wholegraph_amd.torch as wgth
    for t in ts:
        wgth.destroy_wholememory_tensor(t)


def _structure(comm, col_dtype=np.int64):
    import wholegraph_amd.torch as wgth
    row_ptr, col, weights, _ = walk_ref.ladder()
    ts = [_wm_array(comm, "chunked", row_ptr), _wm_array(comm, "chunked", col.astype(col_dtype)), _wm_array(comm, "chunked", weights)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("w", ts[2])
    return g, ts


def reference(weighted, seed=SEED):
    """walks of the reference -> sorted distinct nodes -> the reference's induced subgraph (computed once, shared)"""
    key = (weighted, seed)
    if key not in _CACHE:
        row_ptr, col, weights, starts = walk_ref.ladder()
        if weighted:
            walks, _ = walk_ref.weighted_walks(row_ptr, col, weights, starts, STEPS, seed)
        else:
            walks, _ = walk_ref.uniform_walks(row_ptr, col, starts, STEPS, seed)
        nodes = np.unique(walks[walks >= 0])
        _CACHE[key] = (nodes,) + isub_ref.induced_subgraph(row_ptr, col, nodes)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("col_dtype", ["int32", "int64"])
def test_saint_sampler_equals_the_composition_of_the_references(gpu_env, weighted, col_dtype):
    import torch
    np_dtype = {"int32": np.int32, "int64": np.int64}[col_dtype]
    g, ts = _structure(gpu_env, np_dtype)
    starts = torch.from_numpy(np.array(walk_ref.ladder()[3])).cuda()
    want = reference(weighted)
    assert want[0].shape[0] >= 600 and want[1][-1] >= 1000, "the walks visit too little of the ladder"
    kw = dict(random_seed=SEED, weight_name="w" if weighted else None)
    got = g.saint_random_walk_subgraph(starts, STEPS, need_edge_output=True, **kw)
    assert len(got) == 4 and got[0].dtype == getattr(torch, col_dtype)
    for name, a, b in zip(("nodes", "offsets", "col", "edge ids"), got, (want[0].astype(np_dtype),) + want[1:]):
        assert a.dtype == torch.from_numpy(np.empty(0, dtype=b.dtype)).dtype and np.array_equal(a.cpu().numpy(), b), name
    three = g.saint_random_walk_subgraph(starts, STEPS, **kw)
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, got)), "two calls with one seed differ"
    other = g.saint_random_walk_subgraph(starts, STEPS, random_seed=SEED + 1, weight_name=kw["weight_name"])
    assert not (other[0].shape == got[0].shape and torch.equal(other[0], got[0])), "another seed, the same node set"
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ the model
def _model(comm, name):
    import torch
    import wholegraph_amd.torch as wgth
    g, ts = _structure(comm)
    emb = wgth.create_embedding(comm, "chunked", "cuda", torch.float32, [N, DIM])
    table = torch.randn(N, DIM, generator=torch.Generator().manual_seed(3))
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(table.cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "sgd", {})
    torch.cuda.synchronize()
    wgth.set_framework("cugraph")
    torch.manual_seed(5)
    args = types.SimpleNamespace(model=name, hiddensize=64, layernum=2, classnum=CLASSES, dropout=0.1, heads=2)
    model = wgth.SubgraphGNNModel(g, emb, args).cuda()

    def done():
        wgth.destroy_wholememory_optimizer(wm_opt)
        wgth.destroy_embedding(emb)
        _destroy(ts)
    return model, emb, wm_opt, done


@pytest.mark.parametrize("name", ["sage", "gat"])
def test_model_forward_equals_its_layers_by_hand_on_the_reference_block(gpu_env, name):
    import torch
    import torch.nn.functional as F
    import wholegraph_amd.torch as wgth
    model, emb, _, done = _model(gpu_env, name)
    kinds = {"sage": "CuGraphSAGEConv", "gat": "CuGraphGATConv"}
    assert [type(l).__name__ for l in model.gnn_layers] == [kinds[name]] * 2 and model.add_self_loop == (name == "gat")
    if name == "gat":
        assert [(l.heads, l.concat, l.out_channels) for l in model.gnn_layers] == [(2, True, 32), (2, False, CLASSES)]
    nodes_np, offsets_np, col_np, _ = reference(False)
    nodes, offsets, col = (torch.from_numpy(np.array(a)).cuda() for a in (nodes_np, offsets_np, col_np))
    model.eval()
    with torch.no_grad():
        got = model(nodes, offsets, col)
        x = emb.gather(nodes, force_dtype=torch.float32)
        row, ind = (offsets, col) if name == "sage" else wgth.graph_ops.add_csr_self_loop(offsets, col)
        x = F.relu(model.gnn_layers[0](x, row, ind, 0))
        want = model.gnn_layers[1](x, row, ind, 0)
        # ... and from the op's own block, which is the reference's
        sampled = model.graph_structure.induced_subgraph(nodes)
        assert torch.equal(sampled[0], offsets) and torch.equal(sampled[1], col)
        again = model(nodes, *sampled)
    assert tuple(got.shape) == (nodes.shape[0], CLASSES) and torch.isfinite(got).all()
    assert torch.equal(got, want), "the forward is not its layers on the block"
    assert torch.equal(got, again)
    done()


@pytest.mark.parametrize("name", ["sage", "gat"])
def test_backward_reaches_the_embedding_and_every_layer_parameter(gpu_env, name):
    import torch
    import torch.nn.functional as F
    model, emb, wm_opt, done = _model(gpu_env, name)
    starts = torch.from_numpy(np.array(walk_ref.ladder()[3])).cuda()
    nodes, offsets, col = model.graph_structure.saint_random_walk_subgraph(starts, STEPS, random_seed=SEED)
    before = emb.get_embedding_tensor().get_local_tensor()[0].clone()
    model.train()
    logits = model(nodes, offsets, col)
    labels = (nodes % CLASSES).long()
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    assert torch.isfinite(loss)
    assert len(emb.sparse_grads) == 1 and torch.equal(emb.sparse_indices[0], nodes)
    grad = emb.sparse_grads[0]
    assert tuple(grad.shape) == (nodes.shape[0], DIM) and torch.isfinite(grad).all() and (grad != 0).any(dim=1).float().mean() > 0.5
    params = dict(model.named_parameters())
    assert len(params) >= 4
    for pname, p in params.items():
        if not p.requires_grad:      # (the embedding's autograd anchor)
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any(), pname
    wm_opt.step(0.1)
    torch.cuda.synchronize()
    after = emb.get_embedding_tensor().get_local_tensor()[0]
    changed = (after != before).any(dim=1)
    assert changed[nodes.long()].float().mean() > 0.5, "the gradients did not reach the table"
    untouched = torch.ones(N, dtype=torch.bool, device="cuda")
    untouched[nodes.long()] = False
    assert not changed[untouched].any(), "rows outside the subgraph changed"
    done()
