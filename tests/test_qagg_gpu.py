"""`gather_agg_concat` over an 8-bit row-quantized table on the MI355X: agg_concat whose rows are read, and dequantized, from
the table by global id (wholegraph_amd/torch/gather_aggregation.py -> csrc/aggregate.cpp -> csrc/kernels/agg_quant.hip;
header section 2j).

Every comparison is bitwise (int32 views). The primary oracle is the composition of two ops that exist without this kernel,
agg_concat(qtable.gather(node_ids), row_ptr, col_ind, aggr). The second one, on one small case per aggregator, is a numpy
float32 restatement written here from the table's raw bytes: np.float32(code) * scale + bias with separately rounded
operations, sequential float32 adds from -0.0 in edge order, the mean as a product with np.float32(1) / np.float32(deg).
The block every case shares has a target of each degree around the batch of 8 edges and around every group width, a target
that is its own neighbour, duplicate node ids, and the first and the last row of the table among them."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest

from test_qrows_gpu import destroy, dev, make_table, raw_of, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
DIMS = [1, 4, 7, 64, 128, 256, 300]   # one dword; a ragged last dword; 16 / 32 / 64 lanes; > 64 dwords (column blocks)
DEGREES = [0, 1, 7, 8, 9, 15, 16, 17, 33, 65, 200]
N_ROWS, N_SRC = 1500, 400
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def ladder_block(n_src=N_SRC, seed=0):
    """(row_ptr, col): every degree of DEGREES twice, in a shuffled order, and target 2 (9 edges) among its own neighbours"""
    rng = np.random.default_rng(seed)
    deg = np.array(DEGREES * 2)
    rng.shuffle(deg)
    deg = np.insert(deg, 2, 9)
    row_ptr = np.zeros(len(deg) + 1, np.int32)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n_src, int(row_ptr[-1])).astype(np.int32)
    col[row_ptr[2] + 4] = 2
    for a in (row_ptr, col):
        a.setflags(write=False)
    return row_ptr, col


@functools.lru_cache(maxsize=None)
def node_ids(n_rows, n_src=N_SRC):
    """ids with duplicates, the first and the last row of the table among the targets and among the neighbours"""
    rng = np.random.default_rng(n_rows + n_src)
    ids = rng.integers(0, n_rows, n_src)
    ids[:4] = [0, n_rows - 1, 0, 5]
    ids[-3:] = [n_rows - 1, 5, 5]
    ids.setflags(write=False)
    return ids


def same_bits(a, b):
    import torch
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


def composition(t, ids, rp, ci, aggr):
    from wholegraph_amd.torch.aggregation import agg_concat
    return agg_concat(t.gather(ids), rp, ci, aggr)


def check_fused(t, ids_np, row_ptr, col, aggrs=("sum", "mean"), id_dtypes=(np.int64, np.int32)):
    """the fused op == the composition for every aggregator and id type, one fused forward per call; returns {aggr: out}"""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    assert gather_aggregation.takes_fused_route(t)
    rp, ci = dev(row_ptr), dev(col)
    outs = {}
    for aggr in aggrs:
        for idt in id_dtypes:
            ids = dev(ids_np.astype(idt))
            before = gather_aggregation.quantized_calls()
            got = wgth.gather_agg_concat(t, ids, rp, ci, aggr)
            assert gather_aggregation.quantized_calls() == before + 1, "the fused kernel did not run"
            assert got.dtype == torch.float32 and got.shape == (len(row_ptr) - 1, 2 * t.shape[1])
            assert not got.requires_grad and got.grad_fn is None
            assert same_bits(got, composition(t, ids, rp, ci, aggr)), (aggr, idt)
            outs[aggr] = got
    return outs


# ---------------------------------------------------------------- 1 the grid: width x table type x row alignment
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mt,row_align", [("continuous", 16), ("chunked", 16), ("chunked", 4)])
def test_forward_bitwise(gpu_env, mt, row_align, dim):
    import wholegraph_amd.torch as wgth
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, mt, "cuda", x, row_align=row_align)
    rb = wgth.quantized_row_bytes(dim)
    assert t.storage.stride()[0] == (rb + row_align - 1) // row_align * row_align   # (dim 128, align 4: 136 bytes)
    row_ptr, col = ladder_block()
    outs = check_fused(t, node_ids(N_ROWS), row_ptr, col)
    empty = np.nonzero(np.diff(row_ptr) == 0)[0]
    assert len(empty) == 2
    for aggr in outs:   # a target without edges: +0.0 in the aggregate half
        assert np.array_equal(outs[aggr][empty, :dim].cpu().numpy().view(np.uint32), np.zeros((2, dim), np.uint32))
    destroy(t)


# ---------------------------------------------------------------- 2 the arithmetic, restated
def numpy_forward(raw, dim, ids_np, row_ptr, col, aggr):
    """raw: uint8 [N, >= Q + 8], the table's bytes"""
    q = (dim + 3) // 4 * 4
    codes = raw[:, :dim].astype(F32)
    scale = np.ascontiguousarray(raw[:, q:q + 4]).view(F32)[:, 0]
    bias = np.ascontiguousarray(raw[:, q + 4:q + 8]).view(F32)[:, 0]
    assert codes.dtype == F32 and scale.dtype == F32 and bias.dtype == F32

    def row(i):
        r = ids_np[i]
        prod = codes[r] * scale[r]          # float32 * float32 -> float32: rounded on its own
        return prod + bias[r]

    n_dst = len(row_ptr) - 1
    out = np.zeros((n_dst, 2 * dim), F32)
    for d in range(n_dst):
        e0, e1 = int(row_ptr[d]), int(row_ptr[d + 1])
        acc = np.full(dim, -0.0, F32)
        for e in range(e0, e1):
            acc = acc + row(col[e])
        if e1 == e0:
            acc = np.zeros(dim, F32)
        elif aggr == "mean":
            acc = acc * (F32(1) / F32(e1 - e0))
        assert acc.dtype == F32
        out[d, :dim] = acc
        out[d, dim:] = row(d)
    return out


@pytest.mark.parametrize("aggr", ["sum", "mean"])
def test_against_the_numpy_restatement(gpu_env, aggr):
    import torch
    for dim in (7, 128):
        x, _, _ = reference(N_ROWS, dim)
        t = make_table(gpu_env, "chunked", "cuda", x, row_align=4)
        raw = raw_of(t).cpu().numpy().view(np.uint8)
        row_ptr, col = ladder_block()
        ids_np = node_ids(N_ROWS)
        got = check_fused(t, ids_np, row_ptr, col, aggrs=(aggr,), id_dtypes=(np.int64,))[aggr]
        want = numpy_forward(raw, dim, ids_np, row_ptr, col, aggr)
        assert same_bits(got, torch.from_numpy(want)), dim
        destroy(t)


# ---------------------------------------------------------------- 3 shapes of blocks, views, special rows
def test_block_whose_every_node_is_a_target(gpu_env):
    """n_src == n_dst, and the degenerate blocks: no edge at all, no target at all"""
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    dim = 64
    x, _, _ = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x)
    row_ptr, col = ladder_block(n_src=len(DEGREES) * 2 + 1, seed=1)
    n = len(row_ptr) - 1
    ids_np = np.array(node_ids(N_ROWS)[:n])
    assert int(col.max()) < n and len(ids_np) == n
    check_fused(t, ids_np, row_ptr, col)
    out = check_fused(t, ids_np, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), aggrs=("mean",))["mean"]
    assert np.array_equal(out[:, :dim].cpu().numpy().view(np.uint32), np.zeros((n, dim), np.uint32))
    for n_src in (n, 0):
        before = gather_aggregation.quantized_calls()
        out = wgth.gather_agg_concat(t, dev(ids_np[:n_src]), dev(np.zeros(1, np.int32)), dev(np.zeros(0, np.int32)), "sum")
        assert out.shape == (0, 2 * dim) and gather_aggregation.quantized_calls() == before + 1
    destroy(t)


@pytest.mark.parametrize("dim,row_align", [(7, 4), (128, 4), (128, 16)])
def test_row_range_view_with_a_storage_offset(gpu_env, dim, row_align):
    import wholegraph_amd.torch as wgth
    x, _, _ = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=row_align)
    r0, r1 = 101, 1301
    view = wgth.WholeMemoryQuantizedTensor(t.storage.get_sub_tensor([r0, 0], [r1, -1]), dim)
    assert view.shape == (r1 - r0, dim) and view.storage.storage_offset() == r0 * t.storage.stride()[0] > 0
    row_ptr, col = ladder_block()
    outs = check_fused(view, node_ids(r1 - r0), row_ptr, col)
    # ... and the view's row i is the table's row r0 + i
    shifted = check_fused(t, np.array(node_ids(r1 - r0)) + r0, row_ptr, col, id_dtypes=(np.int64,))
    for aggr in outs:
        assert same_bits(outs[aggr], shifted[aggr])
    destroy(t)


def test_constant_rows_and_rows_with_the_extreme_codes(gpu_env):
    """a constant row is scale 1.0 and every code 0 (its values come from the bias alone, a zero row's are +0.0); a row with
    a spread holds code 0 at its minimum and code 255 at its maximum"""
    import torch
    dim, n = 128, 64
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n, dim)).astype(F32)
    x[0::4] = (rng.standard_normal(n // 4) * 100.0).astype(F32)[:, None]
    x[4] = 0.0
    x[8] = -0.0
    t = make_table(gpu_env, "continuous", "cuda", x, row_align=4)
    raw = raw_of(t).cpu().numpy().view(np.uint8)
    const = np.arange(n) % 4 == 0
    assert not raw[const, :dim].any() and (np.ascontiguousarray(raw[const, dim:dim + 4]).view(F32) == 1.0).all()
    assert (raw[~const, :dim].min(axis=1) == 0).all() and (raw[~const, :dim].max(axis=1) == 255).all()
    row_ptr, col = ladder_block(n_src=n, seed=2)
    ids_np = np.random.default_rng(10).permutation(n)
    for aggr, got in check_fused(t, ids_np, row_ptr, col).items():
        assert same_bits(got, torch.from_numpy(numpy_forward(raw, dim, ids_np, row_ptr, col, aggr))), aggr
    # a block whose every row is a zero row: sums of +0.0 from -0.0 are +0.0
    zeros = np.where(np.arange(n) % 2 == 0, 4, 8)
    out = check_fused(t, zeros, row_ptr, col, aggrs=("sum",), id_dtypes=(np.int64,))["sum"]
    assert not out.cpu().numpy().view(np.uint32).any()
    destroy(t)


# ---------------------------------------------------------------- 4 the element-wise store path from aligned widths
def qagg_into(t, ids, rp, ci, n_edges, n_dst, n_src, aggr_code, out, stride):
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import get_stream, get_wholegraph_env_fns
    return wmb.lib().wholememory_ext_csc_gather_dequantize_aggregate_forward(
        t.storage.wmb_tensor, t.shape[1], C.c_void_p(ids.data_ptr()), wmb.DT_INT64, C.c_void_p(rp.data_ptr()),
        C.c_void_p(ci.data_ptr()), n_edges, n_dst, n_src, aggr_code, C.c_void_p(out.data_ptr()), stride,
        get_wholegraph_env_fns(), C.c_void_p(get_stream()))


@pytest.mark.parametrize("dim", [64, 128, 256, 7])
@pytest.mark.parametrize("pad", [1, 4])
def test_strided_out_through_the_c_abi(gpu_env, dim, pad):
    """out rows 2 * dim + pad floats apart. pad = 1: the rows lose their 16-byte alignment, so the widths that are whole
    dwords take the element-wise stores too; the floats between the rows stay untouched"""
    import torch
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch import gather_aggregation
    x, _, _ = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=4)
    row_ptr, col = ladder_block()
    n_dst = len(row_ptr) - 1
    ids, rp, ci = dev(np.array(node_ids(N_ROWS))), dev(row_ptr), dev(col)
    stride = 2 * dim + pad
    for aggr, code in (("mean", wmb.AGGR_MEAN), ("sum", wmb.AGGR_SUM)):
        out = torch.full((n_dst, stride), SENTINEL, device="cuda")
        before = gather_aggregation.quantized_calls()
        wmb.check(qagg_into(t, ids, rp, ci, len(col), n_dst, N_SRC, code, out, stride))
        assert gather_aggregation.quantized_calls() == before + 1
        torch.cuda.synchronize()
        assert same_bits(out[:, :2 * dim], composition(t, ids, rp, ci, aggr))
        assert bool((out[:, 2 * dim:] == SENTINEL).all()), "floats between the rows were written"
    destroy(t)


# ---------------------------------------------------------------- 5 routes
@pytest.mark.parametrize("mt,loc", [("chunked", "cpu"), ("continuous", "cpu"), ("distributed", "cuda")])
def test_host_and_distributed_tables_take_the_composition(gpu_env, mt, loc):
    """a host-located table (the fused kernel would pull a row across PCIe once per edge) and a DISTRIBUTED one (world size
    1): the same bits, and the fused counter stays still"""
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    dim = 128
    x, _, _ = reference(N_ROWS, dim)
    t = make_table(gpu_env, mt, loc, x)
    fused = make_table(gpu_env, "chunked", "cuda", x)
    assert not gather_aggregation.takes_fused_route(t) and gather_aggregation.takes_fused_route(fused)
    row_ptr, col = ladder_block()
    ids, rp, ci = dev(np.array(node_ids(N_ROWS))), dev(row_ptr), dev(col)
    for aggr in ("sum", "mean"):
        want = wgth.gather_agg_concat(fused, ids, rp, ci, aggr)
        before = gather_aggregation.quantized_calls()
        got = wgth.gather_agg_concat(t, ids, rp, ci, aggr, is_training=True)
        assert gather_aggregation.quantized_calls() == before
        assert same_bits(got, want) and same_bits(got, composition(t, ids, rp, ci, aggr))
    if mt == "distributed":   # the C entry point refuses it and queues nothing
        import torch
        from wholegraph_amd import binding as wmb
        n_dst = len(row_ptr) - 1
        out = torch.full((n_dst, 2 * dim), SENTINEL, device="cuda")
        assert qagg_into(t, ids, rp, ci, len(col), n_dst, N_SRC, wmb.AGGR_SUM, out, 2 * dim) == wmb.NOT_SUPPORTED
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and gather_aggregation.quantized_calls() == before
    destroy(t)
    destroy(fused)


def test_chunked_table_over_two_ranks_sharing_one_device(wm_lib):
    """a CHUNKED table whose halves live in two processes, both ranks on cuda:0 (collectives over gloo): the rows of the
    peer's chunk are read through its mapping, with equal chunks (owner by multiply-high) and with a custom partition (owner
    by search); the ids land on both ranks and on the last row of each"""
    from test_distributed_cpu import free_port
    port = str(free_port())
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_qagg_worker.py"), str(r), "2", port], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("RANK %d OK" % r) in o, "rank %d failed:\n%s" % (
            r, "\n=====\n".join(x[-2500:] for x in outs))


# ---------------------------------------------------------------- 6 the layer and the model
def test_layer_from_a_quantized_table(gpu_env):
    """forward_from_table(qtable) == forward(qtable.gather(ids)) bit for bit, and so are the gradients that reach the
    layer's weights; nothing is queued for the (frozen) table"""
    import torch
    from wholegraph_amd.torch import gather_aggregation
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    dim = 128
    x, _, _ = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=4)
    row_ptr, col = ladder_block()
    ids, rp, ci = dev(np.array(node_ids(N_ROWS))), dev(row_ptr), dev(col)
    torch.manual_seed(0)
    for aggr in ("mean", "sum"):
        layer = CuGraphSAGEConv(dim, 16, aggr=aggr).cuda()
        grads = []
        for is_training in (False, True):
            layer.zero_grad()
            before = gather_aggregation.quantized_calls()
            out = layer.forward_from_table(t, ids, rp, ci, 200, is_training=is_training)
            assert gather_aggregation.quantized_calls() == before + 1
            (out * 1e-3).square().sum().backward()
            grads.append({n: p.grad.clone() for n, p in layer.named_parameters()})
            layer.zero_grad()
            want = layer(t.gather(ids), rp, ci, 200)
            assert same_bits(out, want)
            (want * 1e-3).square().sum().backward()
            assert layer.lin.weight.grad is not None and float(layer.lin.weight.grad.abs().sum()) > 0
            for n, p in layer.named_parameters():
                assert same_bits(grads[-1][n], p.grad), n
    destroy(t)


def _wm_array(comm, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


def test_model_over_a_quantized_table(gpu_env):
    """HomoGNNModel takes a WholeMemoryQuantizedTensor: identical logits with and without fuse_gather in eval mode, layer 0
    from the fused kernel only with the flag; a training step runs on it"""
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    torch.manual_seed(5)
    rng = np.random.default_rng(5)
    n, k, dim, deg = 3000, 3, 32, 12
    labels_np = rng.integers(0, k, n)
    row_ptr = np.arange(n + 1, dtype=np.int64) * deg
    col = rng.integers(0, n, n * deg).astype(np.int64)
    feats = (rng.standard_normal((k, dim))[labels_np] + 0.5 * rng.standard_normal((n, dim))).astype(F32)
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    t = make_table(gpu_env, "chunked", "cuda", feats)
    wgth.set_framework("cugraph")
    models = []
    for flag in (True, False):
        args = types.SimpleNamespace(model="sage", hiddensize=32, layernum=2, classnum=k, dropout=0.0, neighbors="8,8",
                                     inferencesample="8,8", heads=1, fuse_gather=flag)
        models.append(wgth.HomoGNNModel(g, t, args).cuda())
    fused, plain = models
    plain.load_state_dict(fused.state_dict())
    assert fused.fuse_gather and not plain.fuse_gather
    assert fused.gnn_layers[0].in_channels == dim
    ids = torch.arange(0, n, 11, device="cuda")
    with torch.no_grad():
        outs = []
        for model, moves in ((fused, 1), (plain, 0)):
            model.eval()
            random.seed(5)   # (the sampler draws its per-hop seeds from `random`: the same blocks for both models)
            before = gather_aggregation.quantized_calls()
            outs.append(model(ids))
            assert gather_aggregation.quantized_calls() == before + moves
        assert outs[0].shape == (len(ids), k) and same_bits(outs[0], outs[1])
    labels = torch.from_numpy(labels_np).cuda()
    for model in models:
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        random.seed(6)
        loss = Fn.cross_entropy(model(ids), labels[ids])
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None for p in model.parameters())
        opt.step()
        assert bool(torch.isfinite(loss))
    for a, b in zip(fused.parameters(), plain.parameters()):   # the same step on both routes
        assert same_bits(a.detach(), b.detach())
    destroy(t)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)
