"""`gather_agg_concat` on the MI355X: agg_concat whose rows come straight from a WholeMemory table by global id
(wholegraph_amd/torch/gather_aggregation.py -> csrc/kernels/agg_gather.hip; header section 2e).

Every result is compared with torch.equal against two things: a numpy restatement of the order section 2b states, written
here, over the table's rows widened to fp32; and the two-op composition agg_concat(emb.gather(ids, force_dtype=float32)).
All ids are valid rows of their table (the op's contract). Then the training route (the gradients queued on the embedding
and the tables after an optimizer step equal the two-op model's bit for bit), HomoGNNModel with fuse_gather, and a chunked
table whose shards live in two processes."""
import ctypes as C
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
DTYPES = ["float32", "float16", "bfloat16"]
DIMS = [1, 11, 32, 127, 128, 129, 513]


# ---------------------------------------------------------------- the order of section 2b, restated
def ref_forward(row_ptr, col, x, aggr):
    """out[d] = (S(d) [* fl(1/deg)], x[d]); S summed left to right from the first term; +0.0 for an empty target"""
    row_ptr = np.asarray(row_ptr, np.int64)
    n_dst, dim = len(row_ptr) - 1, x.shape[1]
    deg = np.diff(row_ptr)
    out = np.zeros((n_dst, 2 * dim), F32)
    acc = np.zeros((n_dst, dim), F32)
    for k in range(int(deg.max()) if n_dst else 0):   # k-th term of every target that has one: same order per target
        live = np.nonzero(deg > k)[0]
        term = x[col[row_ptr[live] + k]]
        acc[live] = term if k == 0 else acc[live] + term
    if aggr == "mean":
        nz = deg > 0
        acc[nz] = acc[nz] * (F32(1.0) / deg[nz].astype(F32))[:, None]
    acc[deg == 0] = F32(0.0)
    out[:, :dim] = acc
    out[:, dim:] = x[:n_dst]
    return out


def block(rng, n_dst, n_src, max_deg, hub=None, hub_share=0.0, empty_every=7):
    deg = rng.integers(0, max_deg + 1, n_dst)
    deg[::empty_every] = 0
    if n_dst > 3:
        deg[1] = max_deg
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n_src, int(row_ptr[-1])).astype(np.int32)
    if hub is not None:
        col[rng.random(len(col)) < hub_share] = hub
    return row_ptr, col


def table_values(rng, n_rows, dim, dtype):
    """rows whose magnitudes spread over many binades, so that an fp32 sum of them depends on its order also when the
    elements have 8 or 11 significant bits; returned in `dtype` (a torch tensor on the host)"""
    import torch
    v = rng.standard_normal((n_rows, dim)) * np.exp2(rng.integers(-12, 13, (n_rows, dim)))
    return torch.from_numpy(v.astype(F32)).to(dtype)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def make_embedding(comm, mt, loc, dtype, values, **kw):
    """an embedding of `dtype` filled with `values` (host tensor of that dtype) through the library's own scatter"""
    import torch
    import wholegraph_amd.torch as wgth
    n, dim = values.shape
    emb = wgth.create_embedding(comm, mt, loc, dtype, [n, dim], **kw)
    emb.get_embedding_tensor().scatter(values.cuda(), torch.arange(n, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    return emb


def check_both(source, values, ids_np, row_ptr, col, aggr, id_dtype=np.int64, gather_from=None):
    """fused == numpy restatement and fused == agg_concat(gather); returns the fused result"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    from wholegraph_amd.torch.aggregation import agg_concat
    ids = dev(ids_np.astype(id_dtype))
    rp, ci = dev(row_ptr), dev(col)
    before = gather_aggregation.calls()
    got = wgth.gather_agg_concat(source, ids, rp, ci, aggr)
    assert gather_aggregation.calls() == before + 1, "the fused kernel did not run"
    assert got.dtype == torch.float32 and got.shape == (len(row_ptr) - 1, 2 * values.shape[1])
    x_np = values.float().numpy()[ids_np]
    want = torch.from_numpy(ref_forward(row_ptr, col, x_np, aggr))
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    two = agg_concat((gather_from or source).gather(ids, force_dtype=torch.float32), rp, ci, aggr)
    assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    return got


# ---------------------------------------------------------------- 1 forward, every dtype / width / aggregator / id type
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_bitwise(gpu_env, dtype, dim):
    import torch
    import wholegraph_amd.torch as wgth
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(dim * 13 + len(dtype))
    n_rows, n_dst, n_src = 5003, 301, 1000
    values = table_values(rng, n_rows, dim, tdt)
    emb = make_embedding(gpu_env, "chunked", "cuda", tdt, values)
    row_ptr, col = block(rng, n_dst, n_src, 64)
    ids_np = rng.integers(0, n_rows, n_src)
    ids_np[:3] = [0, n_rows - 1, 0]
    for aggr in ("mean", "sum"):
        a = check_both(emb, values, ids_np, row_ptr, col, aggr, np.int64)
        b = check_both(emb, values, ids_np, row_ptr, col, aggr, np.int32)
        assert torch.equal(a, b)
    wgth.destroy_embedding(emb)


# ---------------------------------------------------------------- 2 shapes of blocks
@pytest.mark.parametrize("dtype,dim", [("float32", 128), ("bfloat16", 128), ("float16", 11)])
def test_power_law_block_with_hub(gpu_env, dtype, dim):
    import torch
    import wholegraph_amd.torch as wgth
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(5)
    n_rows, n_dst, n_src = 30011, 2000, 9000
    values = table_values(rng, n_rows, dim, tdt)
    emb = make_embedding(gpu_env, "continuous", "cuda", tdt, values)
    deg = np.minimum((rng.pareto(1.2, n_dst) * 4).astype(np.int64), 3000)
    deg[5] = 5000   # a target with thousands of edges
    row_ptr = np.zeros(n_dst + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n_src, int(row_ptr[-1])).astype(np.int32)
    col[rng.random(len(col)) < 0.3] = 17   # and a source that a third of all edges point at
    ids_np = rng.permutation(n_rows)[:n_src]
    for aggr in ("mean", "sum"):
        check_both(emb, values, ids_np, row_ptr, col, aggr)
    wgth.destroy_embedding(emb)


def test_empty_targets_and_empty_blocks(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    rng = np.random.default_rng(6)
    dim = 24
    values = table_values(rng, 777, dim, torch.float32)
    emb = make_embedding(gpu_env, "chunked", "cuda", torch.float32, values)
    ids_np = rng.integers(0, 777, 50)
    # targets without edges among others (block() empties every 3rd here)
    row_ptr, col = block(rng, 40, 50, 9, empty_every=3)
    out = check_both(emb, values, ids_np, row_ptr, col, "mean")
    empty = np.diff(row_ptr) == 0
    assert empty.any() and np.array_equal(bits(out)[empty][:, :dim], np.zeros((int(empty.sum()), dim), np.uint32))
    # E = 0: every target empty -> (+0.0, x[d])
    out = check_both(emb, values, ids_np, np.zeros(6, np.int32), np.zeros(0, np.int32), "sum")
    assert np.array_equal(bits(out[:, :dim]), np.zeros((5, dim), np.uint32))
    assert torch.equal(out[:, dim:].cpu(), values[ids_np[:5]])
    # n_dst = 0 (with and without node ids)
    for n_src in (50, 0):
        before = gather_aggregation.calls()
        out = wgth.gather_agg_concat(emb, dev(ids_np[:n_src].astype(np.int64)), dev(np.zeros(1, np.int32)),
                                     dev(np.zeros(0, np.int32)), "mean")
        assert out.shape == (0, 2 * dim) and gather_aggregation.calls() == before + 1
    wgth.destroy_embedding(emb)


# ---------------------------------------------------------------- 3 views, strides, locations
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c0,c1", [(4, 36), (8, 40), (3, 36), (1, 33)])
def test_subtensor_view_with_column_offset(gpu_env, dtype, c0, c1):
    """a view [r0:r1, c0:c1] of a [N, 40] table: storage offset and row stride come from the tensor description. (8, 40) keeps
    every row start 16-byte aligned for each dtype, (4, 36) for fp32 only; the other two take the element-wise path."""
    import torch
    import wholegraph_amd.torch as wgth
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(c0 * 41 + c1)
    n_rows, r0, r1 = 2003, 101, 1901
    values = table_values(rng, n_rows, 40, tdt)
    emb = make_embedding(gpu_env, "chunked", "cuda", tdt, values)
    view = emb.get_embedding_tensor().get_sub_tensor([r0, c0], [r1, c1])
    assert view.shape == (r1 - r0, c1 - c0) and view.stride()[0] == 40 and view.storage_offset() == r0 * 40 + c0
    row_ptr, col = block(rng, 120, 500, 30)
    ids_np = rng.integers(0, r1 - r0, 500)
    ids_np[:2] = [0, r1 - r0 - 1]
    sub_values = values[r0:r1, c0:c1].contiguous()
    for aggr in ("mean", "sum"):
        check_both(view, sub_values, ids_np, row_ptr, col, aggr)
    wgth.destroy_embedding(emb)


@pytest.mark.parametrize("dtype,dim", [("float32", 32), ("bfloat16", 64), ("float32", 7)])
@pytest.mark.parametrize("pad", [4, 5])
def test_strided_out_through_the_c_abi(gpu_env, dtype, dim, pad):
    """out rows 2F + pad floats apart (pad = 5: rows lose their 16-byte alignment); the columns behind 2F stay untouched"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import get_stream, get_wholegraph_env_fns
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(dim + pad)
    values = table_values(rng, 1500, dim, tdt)
    emb = make_embedding(gpu_env, "chunked", "cuda", tdt, values)
    n_dst, n_src = 77, 300
    row_ptr, col = block(rng, n_dst, n_src, 25)
    ids_np = rng.integers(0, 1500, n_src)
    ids, rp, ci = dev(ids_np.astype(np.int64)), dev(row_ptr), dev(col)
    stride = 2 * dim + pad
    out = torch.full((n_dst, stride), -7.0, device="cuda")
    wmb.check(wmb.lib().wholememory_ext_csc_gather_aggregate_forward(
        emb.get_embedding_tensor().wmb_tensor, C.c_void_p(ids.data_ptr()), wmb.DT_INT64, C.c_void_p(rp.data_ptr()),
        C.c_void_p(ci.data_ptr()), len(col), n_dst, n_src, wmb.AGGR_MEAN, C.c_void_p(out.data_ptr()), stride,
        get_wholegraph_env_fns(), C.c_void_p(get_stream())))
    torch.cuda.synchronize()
    want = ref_forward(row_ptr, col, values.float().numpy()[ids_np], "mean")
    assert np.array_equal(bits(out[:, :2 * dim].contiguous()), want.view(np.uint32))
    assert bool((out[:, 2 * dim:] == -7.0).all())
    wgth.destroy_embedding(emb)


@pytest.mark.parametrize("mt", ["chunked", "continuous"])
@pytest.mark.parametrize("dtype,dim", [("float32", 128), ("float16", 129)])
def test_host_located_table(gpu_env, mt, dtype, dim):
    import torch
    import wholegraph_amd.torch as wgth
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(dim)
    values = table_values(rng, 3001, dim, tdt)
    emb = make_embedding(gpu_env, mt, "cpu", tdt, values)
    row_ptr, col = block(rng, 150, 600, 30)
    ids_np = rng.integers(0, 3001, 600)
    for aggr in ("mean", "sum"):
        check_both(emb, values, ids_np, row_ptr, col, aggr)
    wgth.destroy_embedding(emb)


def test_wholememory_tensor_source_and_fallback_routes(gpu_env):
    """a plain WholeMemoryTensor is a source too; a DISTRIBUTED table and an embedding behind a cache policy take the two-op
    composition: identical results, the counter does not move"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    rng = np.random.default_rng(8)
    n_rows, dim = 4001, 32
    values = table_values(rng, n_rows, dim, torch.float32)
    row_ptr, col = block(rng, 90, 400, 20)
    ids_np = rng.integers(0, n_rows, 400)
    ids, rp, ci = dev(ids_np.astype(np.int64)), dev(row_ptr), dev(col)
    want = ref_forward(row_ptr, col, values.numpy()[ids_np], "mean").view(np.uint32)
    t = wgth.create_wholememory_tensor(gpu_env, "continuous", "cuda", [n_rows, dim], torch.float32, None)
    t.scatter(values.cuda(), torch.arange(n_rows, device="cuda"))
    assert gather_aggregation.takes_fused_route(t)
    check_both(t, values, ids_np, row_ptr, col, "mean")
    wgth.destroy_wholememory_tensor(t)
    dist_emb = make_embedding(gpu_env, "distributed", "cuda", torch.float32, values)
    policy = wgth.create_wholememory_cache_policy(gpu_env, memory_type="chunked", memory_location="cuda",
                                                  access_type="readonly", ratio=0.3)
    cached = make_embedding(gpu_env, "chunked", "cuda", torch.float32, values, cache_policy=policy)
    for emb in (dist_emb, cached):
        assert not gather_aggregation.takes_fused_route(emb)
        before = gather_aggregation.calls()
        out = wgth.gather_agg_concat(emb, ids, rp, ci, "mean")
        assert gather_aggregation.calls() == before
        assert np.array_equal(bits(out), want)
    wgth.destroy_embedding(dist_emb)
    wgth.destroy_embedding(cached)
    wgth.destroy_wholememory_cache_policy(policy)


# ---------------------------------------------------------------- 4 real sampler output
def _wm_array(comm, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("dtype", DTYPES)
def test_on_sampler_blocks(gpu_env, dtype):
    import torch
    import wholegraph_amd.torch as wgth
    from test_graph_oracle import make_csr
    from wholegraph_amd.torch import gather_aggregation
    from wholegraph_amd.torch.aggregation import agg_concat
    tdt = getattr(torch, dtype)
    n_nodes, dim = 20011, 64
    row_ptr, col = make_csr(n_nodes, 70, 41, np.int64, heavy=[(3, 4000), (4, 0)])
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    values = table_values(np.random.default_rng(12), n_nodes, dim, tdt)
    emb = make_embedding(gpu_env, "chunked", "cuda", tdt, values)
    seeds = torch.from_numpy(np.random.default_rng(3).permutation(n_nodes)[:512].astype(np.int64)).cuda()
    seeds[:2] = torch.tensor([3, 4])
    target_gids, _, csr_row_ptr, csr_col_ind = g.multilayer_sample_without_replacement(seeds, [30, 30], random_seeds=[7, 8])
    for hop in range(2):   # (hop 0 is layer 0's block; hop 1 is a smaller block of the same kind)
        gids, rp, ci = target_gids[hop], csr_row_ptr[hop], csr_col_ind[hop]
        assert int(gids.min()) >= 0 and int(gids.max()) < n_nodes
        for aggr in ("mean", "sum"):
            before = gather_aggregation.calls()
            got = wgth.gather_agg_concat(emb, gids, rp, ci, aggr)
            assert gather_aggregation.calls() == before + 1
            x_np = values.float().numpy()[gids.cpu().numpy()]
            assert np.array_equal(bits(got), ref_forward(rp.cpu().numpy(), ci.cpu().numpy(), x_np, aggr).view(np.uint32))
            two = agg_concat(emb.gather(gids, force_dtype=torch.float32), rp, ci, aggr)
            assert torch.equal(got.view(torch.int32), two.view(torch.int32))
    wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


# ---------------------------------------------------------------- 5 training route and the model
def _planted_partition(n, k, rng, deg=12, p_in=0.9):
    comm_of = rng.integers(0, k, n)
    members = [np.nonzero(comm_of == c)[0] for c in range(k)]
    rows = []
    for v in range(n):
        same = rng.random(deg) < p_in
        nbr = np.where(same, rng.choice(members[comm_of[v]], deg), rng.integers(0, n, deg))
        rows.append(np.unique(nbr[nbr != v]))
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    return row_ptr, np.concatenate(rows).astype(np.int64), comm_of


def _model_pair(gpu_env, n, k, dim, feats, g, fused_flags, **emb_kw):
    """one HomoGNNModel per flag (None: the attribute is absent) over embeddings with the same rows, an Adam optimizer with
    weight decay each, and the same initial layer weights"""
    import torch
    import wholegraph_amd.torch as wgth
    wgth.set_framework("cugraph")
    made = []
    state = None
    for flag in fused_flags:
        emb = make_embedding(gpu_env, "chunked", "cuda", torch.float32, feats, **emb_kw)
        wm_opt = wgth.create_wholememory_optimizer(emb, "adam", {"weight_decay": 0.01})
        args = types.SimpleNamespace(model="sage", hiddensize=64, layernum=2, classnum=k, dropout=0.0, neighbors="10,10",
                                     inferencesample="10,10", heads=1)
        if flag is not None:
            args.fuse_gather = flag
        model = wgth.HomoGNNModel(g, emb, args).cuda()
        if state is None:
            state = {name: v.clone() for name, v in model.state_dict().items()}
        else:
            model.load_state_dict(state)
        made.append((model, emb, wm_opt))
    return made


def test_training_route_and_model_match_the_two_op_model_bit_for_bit(gpu_env):
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    torch.manual_seed(1)
    rng = np.random.default_rng(2)
    n, k, dim = 4000, 4, 32
    row_ptr, col, labels_np = _planted_partition(n, k, rng)
    feats = torch.from_numpy((0.5 * rng.standard_normal((k, dim))[labels_np] + rng.standard_normal((n, dim))).astype(F32))
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    labels = torch.from_numpy(labels_np).cuda()
    (fused, emb_f, opt_f), (plain, emb_p, opt_p), (default, emb_d, opt_d) = _model_pair(gpu_env, n, k, dim, feats, g,
                                                                                       (True, False, None))
    assert fused.fuse_gather and not plain.fuse_gather and not default.fuse_gather
    all_ids = torch.arange(n, dtype=torch.int64, device="cuda")
    for step in range(3):
        ids = torch.from_numpy(rng.choice(n, 256, replace=False).astype(np.int64)).cuda()
        results = []
        for model, emb, wm_opt, moves in ((fused, emb_f, opt_f, 1), (plain, emb_p, opt_p, 0), (default, emb_d, opt_d, 0)):
            model.train()
            random.seed(1000 + step)   # the sampler draws its per-hop seeds from `random`: the same blocks for every model
            before = gather_aggregation.calls()
            logits = model(ids)
            assert gather_aggregation.calls() == before + moves   # one fused forward per model forward, none with the flag off
            loss = Fn.cross_entropy(logits, labels[ids])
            model.zero_grad()
            loss.backward()
            assert emb.need_apply and len(emb.sparse_indices) == 1 and len(emb.sparse_grads) == 1
            queued = (emb.sparse_indices[0].clone(), emb.sparse_grads[0].clone())
            grads = {name: p.grad.clone() for name, p in model.named_parameters() if p.grad is not None}
            wm_opt.step(0.05)
            assert not emb.need_apply and not emb.sparse_indices
            with torch.no_grad():   # (plain SGD on the layers, the same arithmetic for every model)
                for p in model.parameters():
                    if p.grad is not None:
                        p -= 0.05 * p.grad
            torch.cuda.synchronize()
            results.append((logits.detach().clone(), queued, grads, emb.gather(all_ids).clone()))
        ref = results[1]
        for got in (results[0], results[2]):
            assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), "logits differ at step %d" % step
            assert torch.equal(got[1][0], ref[1][0]), "queued ids differ"
            assert got[1][1].dtype == torch.float32 and got[1][1].shape == ref[1][1].shape
            assert torch.equal(got[1][1].view(torch.int32), ref[1][1].view(torch.int32)), "queued row gradients differ"
            assert got[2].keys() == ref[2].keys()
            for name in ref[2]:
                assert torch.equal(got[2][name].view(torch.int32), ref[2][name].view(torch.int32)), name
            assert torch.equal(got[3].view(torch.int32), ref[3].view(torch.int32)), "tables differ after the optimizer step"
        assert not torch.equal(ref[3].cpu(), feats), "the optimizer step changed nothing"
    # inference: no backward work is queued, the logits still agree
    with torch.no_grad():
        ids = torch.arange(0, n, 16, device="cuda")
        outs = []
        for model, emb in ((fused, emb_f), (plain, emb_p)):
            model.eval()
            random.seed(77)
            outs.append(model(ids))
            assert not emb.need_apply and not emb.sparse_indices
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    for model, emb, wm_opt in ((fused, emb_f, opt_f), (plain, emb_p, opt_p), (default, emb_d, opt_d)):
        wgth.destroy_wholememory_optimizer(wm_opt)
        wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


def test_frozen_features_queue_no_backward_work(gpu_env):
    """without an optimizer (or outside training) the backward hands nothing to the embedding; the layer's own parameters
    still receive their gradients"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    rng = np.random.default_rng(4)
    values = table_values(rng, 2000, 48, torch.bfloat16)
    emb = make_embedding(gpu_env, "chunked", "cuda", torch.bfloat16, values)
    row_ptr, col = block(rng, 100, 500, 20)
    ids = dev(rng.integers(0, 2000, 500))
    torch.manual_seed(0)
    layer = CuGraphSAGEConv(48, 16).cuda()
    for is_training in (False, True):
        layer.zero_grad()
        out = layer.forward_from_table(emb, ids, dev(row_ptr), dev(col), 20, is_training=is_training)
        want = layer(emb.gather(ids, force_dtype=torch.float32), dev(row_ptr), dev(col), 20)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        out.square().sum().backward()
        assert layer.lin.weight.grad is not None and layer.lin.weight.grad.abs().sum() > 0
        assert not emb.need_apply and not emb.sparse_indices and not emb.sparse_grads
    wgth.destroy_embedding(emb)


def test_model_on_a_cached_embedding_falls_back(gpu_env):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    n, k, dim = 3000, 3, 16
    row_ptr, col, _ = _planted_partition(n, k, rng)
    feats = torch.from_numpy(rng.standard_normal((n, dim)).astype(F32))
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    policy = wgth.create_wholememory_cache_policy(gpu_env, memory_type="chunked", memory_location="cuda",
                                                  access_type="readonly", ratio=0.3)
    wgth.set_framework("cugraph")
    args = types.SimpleNamespace(model="sage", hiddensize=32, layernum=2, classnum=k, dropout=0.0, neighbors="8,8",
                                 inferencesample="8,8", heads=1, fuse_gather=True)
    cached = make_embedding(gpu_env, "chunked", "cuda", torch.float32, feats, cache_policy=policy)
    plain_emb = make_embedding(gpu_env, "chunked", "cuda", torch.float32, feats)
    m_cached = wgth.HomoGNNModel(g, cached, args).cuda().eval()
    m_plain = wgth.HomoGNNModel(g, plain_emb, args).cuda().eval()
    m_plain.load_state_dict(m_cached.state_dict())
    ids = torch.arange(0, n, 11, device="cuda")
    with torch.no_grad():
        before = gather_aggregation.calls()
        random.seed(5)
        a = m_cached(ids)
        assert gather_aggregation.calls() == before        # the cache policy: gather, then agg_concat
        random.seed(5)
        b = m_plain(ids)
        assert gather_aggregation.calls() == before + 1    # the same flag on a plain table: the fused kernel
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    wgth.destroy_embedding(cached)
    wgth.destroy_embedding(plain_emb)
    wgth.destroy_wholememory_cache_policy(policy)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


# ---------------------------------------------------------------- 6 a chunked table in two processes
def _run_two_ranks(mode):
    from test_distributed_cpu import free_port
    port = str(free_port())
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gather_agg_worker.py"), str(r), "2", port, mode],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("RANK %d OK" % r) in o, "rank %d failed:\n%s" % (
            r, "\n=====\n".join(x[-2500:] for x in outs))


def test_chunked_table_over_two_devices(wm_lib):
    """one rank per device: rows of the peer's chunk are read through its mapping, with equal chunks (owner by multiply-high)
    and with a custom partition (owner by search)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (this box has %d)" % torch.cuda.device_count())
    _run_two_ranks("devices")


def test_chunked_table_over_two_ranks_sharing_one_device(wm_lib):
    """the same scenarios with both ranks on cuda:0 (collectives over gloo), so that the peer-chunk resolve also runs where
    only one device is visible"""
    _run_two_ranks("shared")
