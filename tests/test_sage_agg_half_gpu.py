"""GraphSAGE neighbour aggregation on fp16 / bf16 rows on the MI355X (wholegraph_amd/torch/aggregation.py ->
csrc/kernels/agg_half.hip).

The header (include/wholememory/wholegraph_amd_ext.h, section 2b) states the op on 16-bit rows as: the fp32 sums of the
fp32 op, term by term in the same order, and ONE rounding of each output element to T (nearest even). So everything here
is compared bit for bit (uint16 views): against a numpy restatement of that order followed by one rounding
(`astype(np.float16)` for fp16, torch-CPU `.to(torch.bfloat16)` for bf16), against the fp32 op of this library rounded
once, and against bit patterns derived by hand for the rounding edges. Then the layer, a HomoGNNModel trained under
torch.autocast, and the GAT layer under autocast (its op stays fp32)."""
import types

import numpy as np
import pytest

import _long_runs as LR

pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = ["float16", "bfloat16"]


# ---------------------------------------------------------------- 16-bit rows as uint16 bit patterns
def tdtype(name):
    import torch
    return getattr(torch, name)


def round_bits(a, name):
    """round_T of an fp32 array, once, to nearest even: the uint16 bit patterns"""
    import torch
    a = np.ascontiguousarray(a, F32)
    if name == "float16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).view(np.uint16)
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def widen(bits_, name):
    """fp32 values of 16-bit patterns (exact)"""
    if name == "float16":
        return bits_.view(np.float16).astype(F32)
    return (bits_.astype(np.uint32) << 16).view(F32)


def dev16(bits_, name):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits_).view(np.int16)).cuda().view(tdtype(name))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    import torch
    assert t.dtype in (torch.float16, torch.bfloat16)
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def random_rows(rng, shape, name, scale=1.0):
    """(uint16 patterns of T, their exact fp32 values)"""
    b = round_bits((scale * rng.standard_normal(shape)).astype(F32), name)
    return b, widen(b, name)


# ---------------------------------------------------------------- the order, restated (fp32, as for the fp32 op)
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


def ref_backward(row_ptr, col, grad_out, n_src, aggr, chunk):
    """grad_x in fp32: t(e) in fp32; per source the terms in ascending edge position, runs longer than `chunk` cut into
    chunks of that many, each summed left to right, the chunk sums added in chunk order; the self term last. (Sources with
    at most `chunk` edges are advanced together, one term each per step: the same order per source.)"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n_dst, dim = len(row_ptr) - 1, grad_out.shape[1] // 2
    deg = np.diff(row_ptr)
    dst = np.repeat(np.arange(n_dst), deg)
    terms = grad_out[dst, :dim]
    if aggr == "mean":
        terms = terms * (F32(1.0) / deg[dst].astype(F32))[:, None]
    order = np.argsort(col, kind="stable")
    counts = np.bincount(col, minlength=n_src)
    starts = np.concatenate([[0], np.cumsum(counts)])
    P = np.zeros((n_src, dim), F32)
    small = np.nonzero((counts > 0) & (counts <= chunk))[0]
    for k in range(int(counts[small].max()) if len(small) else 0):
        live = small[counts[small] > k]
        t = terms[order[starts[live] + k]]
        P[live] = t if k == 0 else P[live] + t
    for s in np.nonzero(counts > chunk)[0]:
        edges = order[starts[s]:starts[s + 1]]
        p = None
        for c0 in range(0, len(edges), chunk):
            part = terms[edges[c0]].copy()
            for e in edges[c0 + 1:c0 + chunk]:
                part = part + terms[e]
            p = part if p is None else p + part
        P[s] = p
    gx = np.zeros((n_src, dim), F32)
    has = counts > 0
    gx[has] = P[has]
    both = has.copy()
    both[n_dst:] = False
    gx[both] = P[both] + grad_out[both[:n_dst], dim:]
    only_self = ~has
    only_self[n_dst:] = False
    gx[only_self] = grad_out[only_self[:n_dst], dim:]
    return gx


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


def same_bits(got, want, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = got != want
    assert not diff.any(), "%s: %d of %d elements differ, first at %s" % (what, int(diff.sum()), diff.size,
                                                                         tuple(np.argwhere(diff)[0]))


# ---------------------------------------------------------------- 1 forward
@pytest.mark.parametrize("dim", [1, 3, 8, 64, 127, 128, 256, 602])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("name", DTYPES)
def test_forward_bitwise(gpu_env, name, aggr, dim):
    from wholegraph_amd.torch.aggregation import agg_concat
    rng = np.random.default_rng(dim * 7 + len(aggr))
    n_dst, n_src = 301, 1000
    row_ptr, col = block(rng, n_dst, n_src, 64)
    xb, x32 = random_rows(rng, (n_src, dim), name)
    want = round_bits(ref_forward(row_ptr, col, x32, aggr), name)
    same_bits(want[:, dim:], xb[:n_dst], "the restatement copies the targets' rows")
    x = dev16(xb, name)
    out = agg_concat(x, dev(row_ptr), dev(col), aggr)
    assert out.shape == (n_dst, 2 * dim) and out.dtype == tdtype(name)
    same_bits(bits(out), want, "contiguous rows, int32 indices")
    out64 = agg_concat(x, dev(row_ptr.astype(np.int64)), dev(col.astype(np.int64)), aggr)
    same_bits(bits(out64), want, "int64 indices")
    # the same data as a strided view that starts 3 elements (6 bytes) into a wider row: the element-wise path
    wide = np.zeros((n_src, dim + 9), np.uint16)
    wide[:, 3:3 + dim] = xb
    xv = dev16(wide, name)[:, 3:3 + dim]
    assert xv.stride(0) == dim + 9 and xv.data_ptr() % 16 != 0
    same_bits(bits(agg_concat(xv, dev(row_ptr), dev(col), aggr)), want, "strided, offset view")
    # n_dst = 0
    out = agg_concat(x, dev(np.zeros(1, np.int32)), dev(np.zeros(0, np.int32)), aggr)
    assert out.shape == (0, 2 * dim) and out.dtype == tdtype(name)
    # E = 0: every target empty -> (+0.0, x[d])
    out = agg_concat(x, dev(np.zeros(6, np.int32)), dev(np.zeros(0, np.int32)), aggr)
    same_bits(bits(out[:, :dim]), np.zeros((5, dim), np.uint16), "E = 0, aggregate half")
    same_bits(bits(out[:, dim:]), xb[:5], "E = 0, self half")


# ---------------------------------------------------------------- 2 backward
@pytest.mark.parametrize("dim", [1, 3, 8, 64, 127, 128, 602])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("name", DTYPES)
def test_backward_bitwise_with_chunked_hub(gpu_env, name, aggr, dim):
    from wholegraph_amd.torch.aggregation import agg_concat, chunk_edges
    C = chunk_edges()
    assert C >= 1
    rng = np.random.default_rng(100 + dim)
    n_dst, n_src = 300, 1200
    row_ptr, col = block(rng, n_dst, n_src, 64, hub=7, hub_share=0.45)
    col[rng.random(len(col)) < 0.1] = 950      # a second hub, not a target
    counts = np.bincount(col, minlength=n_src)
    assert counts[7] > 3 * C, "the chunked path and the chunk-order combine must run"
    assert (counts == 0).any() and (counts[:n_dst] == 0).any() and (counts[n_dst:] == 0).any()
    xb, _ = random_rows(rng, (n_src, dim), name)
    gb, g32 = random_rows(rng, (n_dst, 2 * dim), name)
    lone = int(np.nonzero(counts[:n_dst] == 0)[0][0])   # a target no edge points at: only its self term
    gb[lone, dim:] = 0x8000                             # -0.0
    g32[lone, dim:] = F32(-0.0)
    gb[5, dim:] = 0x8000
    g32[5, dim:] = F32(-0.0)
    want = round_bits(ref_backward(row_ptr, col, g32, n_src, aggr, C), name)
    same_bits(want[lone], np.full(dim, 0x8000, np.uint16), "a -0.0 self term alone stays -0.0")
    x = dev16(xb, name).requires_grad_(True)
    out = agg_concat(x, dev(row_ptr), dev(col), aggr)
    out.backward(dev16(gb, name))
    assert x.grad.dtype == tdtype(name) and x.grad.shape == (n_src, dim)
    same_bits(bits(x.grad), want, "grad_x")
    # a grad_out with a row stride of its own (the element-wise path when dim is a multiple of 8)
    wide = np.zeros((n_dst, 2 * dim + 5), np.uint16)
    wide[:, 1:1 + 2 * dim] = gb
    x2 = dev16(xb, name).requires_grad_(True)
    agg_concat(x2, dev(row_ptr), dev(col), aggr).backward(dev16(wide, name)[:, 1:1 + 2 * dim])
    same_bits(bits(x2.grad), want, "grad_x from a strided grad_out")
    # E = 0: grad_x = (G[s, F:2F] for s < n_dst, +0.0 after)
    x3 = dev16(xb, name).requires_grad_(True)
    agg_concat(x3, dev(np.zeros(n_dst + 1, np.int32)), dev(np.zeros(0, np.int32)), aggr).backward(dev16(gb, name))
    same_bits(bits(x3.grad[:n_dst]), gb[:, dim:], "E = 0: the self terms")
    same_bits(bits(x3.grad[n_dst:]), np.zeros((n_src - n_dst, dim), np.uint16), "E = 0: rows past the targets")


@pytest.mark.parametrize("dim", [5, 8])
@pytest.mark.parametrize("name", DTYPES)
def test_backward_bitwise_with_runs_of_more_than_one_batch_of_partials(gpu_env, name, dim):
    """runs of 8, 9 and 17 partial rows (tests/_long_runs.py): a full batch, a second pass of the batch loop, a ragged third"""
    from wholegraph_amd.torch.aggregation import agg_concat, chunk_edges
    C = chunk_edges()
    rng = np.random.default_rng(900 + dim)
    row_ptr, col = LR.long_run_block(rng, C)
    LR.assert_long_runs(row_ptr, col, C)
    xb, _ = random_rows(rng, (LR.N_SRC, dim), name)
    gb, g32 = random_rows(rng, (LR.N_DST, 2 * dim), name)
    for aggr in ("mean", "sum"):
        want = round_bits(ref_backward(row_ptr, col, g32, LR.N_SRC, aggr, C), name)
        x = dev16(xb, name).requires_grad_(True)
        agg_concat(x, dev(row_ptr), dev(col), aggr).backward(dev16(gb, name))
        same_bits(bits(x.grad), want, "grad_x, " + aggr)


# ---------------------------------------------------------------- 3 op_T(x) == round_T(op_fp32(fp32(x)))
@pytest.mark.parametrize("name", DTYPES)
def test_identity_with_the_fp32_op_on_power_law_block(gpu_env, name):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    T = tdtype(name)
    rng = np.random.default_rng(5)
    n_dst, n_src, fan, dim = 20000, 120000, 30, 128
    row_ptr = (np.arange(n_dst + 1) * fan).astype(np.int32)
    col = (np.minimum(rng.zipf(1.3, n_dst * fan), n_src) - 1).astype(np.int32)
    assert np.bincount(col).max() > 4000
    rp, ci = dev(row_ptr), dev(col)
    x = dev(rng.standard_normal((n_src, dim)).astype(F32)).to(T).requires_grad_(True)
    g = dev(rng.standard_normal((n_dst, 2 * dim)).astype(F32)).to(T)
    x32 = x.detach().float().requires_grad_(True)
    assert torch.equal(x32.detach().to(T).view(torch.int16), x.detach().view(torch.int16))   # widening is exact
    for aggr in ("mean", "sum"):
        grads = []
        for _ in range(2):
            x.grad = None
            out = agg_concat(x, rp, ci, aggr)
            out.backward(g)
            grads.append(x.grad.clone())
        x32.grad = None
        out32 = agg_concat(x32, rp, ci, aggr)
        out32.backward(g.float())
        assert out.dtype == T and out32.dtype == torch.float32
        same_bits(bits(out), bits(out32.to(T)), "forward %s" % aggr)
        same_bits(bits(grads[0]), bits(x32.grad.to(T)), "backward %s" % aggr)
        same_bits(bits(grads[0]), bits(grads[1]), "two runs of the backward %s" % aggr)


# ---------------------------------------------------------------- 4 rounding edges, expected bits derived by hand
def _edge_block(cases, dim):
    """one target per case with the case's values as its neighbour rows (every column the same); the targets' own rows
    are 1.0. Returns row_ptr, col, fp32 values [n_src, dim]."""
    n_dst = len(cases)
    vals = [1.0] * n_dst
    row_ptr, col = [0], []
    for nbrs in cases:
        for v in nbrs:
            col.append(len(vals))
            vals.append(v)
        row_ptr.append(len(col))
    x = np.repeat(np.array(vals, np.float64)[:, None], dim, axis=1)
    assert np.array_equal(x.astype(F32).astype(np.float64), x)
    return np.array(row_ptr, np.int32), np.array(col, np.int32), x.astype(F32)


@pytest.mark.parametrize("dim", [8, 3])   # the 16-byte and the element-wise instantiation
def test_rounding_edges_fp16(gpu_env, dim):
    from wholegraph_amd.torch.aggregation import agg_concat
    u = 2.0 ** -10   # the spacing of fp16 in [1, 2)
    tiny = 2.0 ** -24   # the smallest fp16 subnormal, 0x0001
    # (neighbour values, aggr, expected fp16 bits of A). fp16: 1 sign, 5 exponent (bias 15), 10 fraction bits
    cases = [
        # ties to even: the fp32 mean is exactly half-way between two fp16 neighbours
        ((1.0, 1.0 + u), "mean", 0x3c00),            # 1 + u/2: between 0x3c00 (even) and 0x3c01 -> down
        ((1.0 + u, 1.0 + 2 * u), "mean", 0x3c02),    # 1 + 3u/2: between 0x3c01 and 0x3c02 (even) -> up
        ((1.0 + 2 * u, 1.0 + 3 * u), "mean", 0x3c02),  # 1 + 5u/2: between 0x3c02 (even) and 0x3c03 -> down
        # not a tie: 1 + 3u/4 is nearer to 1 + u (mean of four)
        ((1.0, 1.0 + u, 1.0 + u, 1.0 + u), "mean", 0x3c01),
        # past the fp16 range: +-inf
        ((40000.0, 40000.0), "sum", 0x7c00),
        ((-40000.0, -40000.0), "sum", 0xfc00),
        ((32768.0, 32736.0), "sum", 0x7bff),         # 65504, the largest finite fp16, exactly
        ((32768.0, 32752.0), "sum", 0x7c00),         # 65520: half-way between 65504 (odd) and 2^16 -> up, to +inf
        ((40000.0, 40000.0), "mean", 0x7800 | 226),  # 40000 = 2^15 + 226 * 32 again: the sum 80000 lived in fp32
        # results in the subnormal range are rounded, not flushed (inputs normal and subnormal)
        ((2.0 ** -14, 0.0), "mean", 0x0200),         # 2^-15 = 512 * 2^-24
        ((2.0 ** -15, 2.0 ** -15), "mean", 0x0200),
        ((tiny, tiny), "sum", 0x0002),
        ((tiny, tiny), "mean", 0x0001),
        ((tiny, 0.0), "mean", 0x0000),               # 2^-25: half-way between 0 (even) and 0x0001 -> +0.0
        ((3 * tiny, 0.0), "mean", 0x0002),           # 1.5 * 2^-24: half-way between 0x0001 and 0x0002 (even)
        ((-3 * tiny, 0.0), "mean", 0x8002),
        ((1023 * tiny, 1024 * tiny), "mean", 0x0400),  # 1023.5 * 2^-24: between 0x03ff and 0x0400 (even): first normal
        # a -0.0-only row stays -0.0 (the sum starts from its first term)
        ((-0.0, -0.0, -0.0), "sum", 0x8000),
        ((-0.0, -0.0, -0.0), "mean", 0x8000),
        ((-0.0, 0.0), "sum", 0x0000),                # -0.0 + +0.0 = +0.0 (round to nearest)
    ]
    row_ptr, col, x32 = _edge_block([c[0] for c in cases], dim)
    xb = x32.astype(np.float16)
    assert np.array_equal(xb.astype(F32).view(np.uint32), x32.view(np.uint32)), "inputs are exact in fp16"
    x = dev16(xb.view(np.uint16), "float16")
    got = {a: bits(agg_concat(x, dev(row_ptr), dev(col), a)) for a in ("mean", "sum")}
    for d, (nbrs, aggr, want) in enumerate(cases):
        row = got[aggr][d]
        assert (row[:dim] == want).all(), "case %d %s of %s: got 0x%04x, want 0x%04x" % (d, aggr, nbrs, row[0], want)
        assert (row[dim:] == 0x3c00).all()


@pytest.mark.parametrize("dim", [8, 3])
def test_rounding_edges_bf16(gpu_env, dim):
    import torch
    from wholegraph_amd.torch.aggregation import agg_concat
    u = 2.0 ** -7   # the spacing of bf16 in [1, 2): 1 sign, 8 exponent (bias 127), 7 fraction bits
    cases = [
        ((1.0, 1.0 + u), "mean", 0x3f80),             # 1 + 2^-8: between 0x3f80 (even) and 0x3f81 -> down
        ((1.0 + u, 1.0 + 2 * u), "mean", 0x3f82),     # 1 + 3 * 2^-8: between 0x3f81 and 0x3f82 (even) -> up
        ((1.0 + 2 * u, 1.0 + 3 * u), "mean", 0x3f82),
        ((1.0, 1.0 + u, 1.0 + u, 1.0 + u), "mean", 0x3f81),   # 1 + 3u/4: nearer to 1 + u
        ((1.0 + u, 1.0 + u, 1.0 + u, 1.0), "sum", 0x4081),    # 4 + 3u, spacing 4u in [4, 8): nearer to 4 + 4u
        ((-0.0, -0.0, -0.0), "sum", 0x8000),
        ((-0.0, -0.0, -0.0), "mean", 0x8000),
        ((2.0 ** -133, 0.0), "mean", 0x0000),         # 2^-134: half-way between 0 and the smallest bf16 subnormal 2^-133
        ((3 * 2.0 ** -133, 0.0), "mean", 0x0002),     # 1.5 * 2^-133: between 0x0001 and 0x0002 (even): not flushed
    ]
    row_ptr, col, x32 = _edge_block([c[0] for c in cases], dim)
    xb = torch.from_numpy(x32).to(torch.bfloat16)
    assert torch.equal(xb.float(), torch.from_numpy(x32)), "inputs are exact in bf16"
    x = xb.cuda()
    got = {a: bits(agg_concat(x, dev(row_ptr), dev(col), a)) for a in ("mean", "sum")}
    for d, (nbrs, aggr, want) in enumerate(cases):
        row = got[aggr][d]
        assert (row[:dim] == want).all(), "case %d %s of %s: got 0x%04x, want 0x%04x" % (d, aggr, nbrs, row[0], want)
        assert (row[dim:] == 0x3f80).all()


# ---------------------------------------------------------------- 5 real sampler output
def _wm_array(comm, arr):
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_wholememory_tensor(comm, "chunked", "cuda", [arr.shape[0]], torch.from_numpy(arr).dtype, [1])
    t.get_local_tensor()[0].copy_(torch.from_numpy(arr))
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name", DTYPES)
def test_on_sampler_blocks(gpu_env, name):
    import torch
    import wholegraph_amd.torch as wgth
    from test_graph_oracle import make_csr
    from wholegraph_amd.torch.aggregation import agg_concat, chunk_edges
    from wholegraph_amd.torch.graph_ops import add_csr_self_loop
    n_nodes, dim = 20011, 64
    row_ptr, col = make_csr(n_nodes, 70, 41, np.int64, heavy=[(3, 4000), (4, 0)])
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    seeds = torch.from_numpy(np.random.default_rng(3).permutation(n_nodes)[:512].astype(np.int64)).cuda()
    seeds[:2] = torch.tensor([3, 4])
    target_gids, _, csr_row_ptr, csr_col_ind = g.multilayer_sample_without_replacement(seeds, [30, 30],
                                                                                       random_seeds=[7, 8])
    rng = np.random.default_rng(9)
    blocks = [(csr_row_ptr[i], csr_col_ind[i], target_gids[i].numel()) for i in range(2)]
    blocks.append(add_csr_self_loop(csr_row_ptr[1], csr_col_ind[1]) + (target_gids[1].numel(),))
    for rp, ci, n_src in blocks:
        assert rp.dtype == torch.int32 and ci.dtype == torch.int32
        rp_np, ci_np = rp.cpu().numpy(), ci.cpu().numpy()
        n_dst = len(rp_np) - 1
        xb, x32 = random_rows(rng, (n_src, dim), name)
        gb, g32 = random_rows(rng, (n_dst, 2 * dim), name)
        x = dev16(xb, name).requires_grad_(True)
        out = agg_concat(x, rp, ci, "mean")
        same_bits(bits(out), round_bits(ref_forward(rp_np, ci_np, x32, "mean"), name), "forward")
        out.backward(dev16(gb, name))
        same_bits(bits(x.grad), round_bits(ref_backward(rp_np, ci_np, g32, n_src, "mean", chunk_edges()), name), "backward")
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


# ---------------------------------------------------------------- 6 CuGraphSAGEConv
@pytest.mark.parametrize("root_weight,project", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("name", DTYPES)
def test_sage_conv_in_16_bit(gpu_env, name, root_weight, project):
    """the layer after .to(T) on T input equals lin(cat) with cat built from the restated forward. Tolerance: one T
    rounding of the GEMM output, rtol = 4 * eps(T) (the factor 4 covers the GEMM's freedom in the order of its own
    accumulation), applied to the scale of each output's sum, sum_k |cat_k| |W_k| + |b| (an output that cancels to
    near zero is still only as accurate as its terms)."""
    import torch
    from wholegraph_amd.torch.cugraphops import CuGraphSAGEConv
    T = tdtype(name)
    torch.manual_seed(0)
    rng = np.random.default_rng(21)
    n_dst, n_src, cin, cout = 150, 700, 48, 24
    row_ptr, col = block(rng, n_dst, n_src, 20)
    rp, ci = dev(row_ptr), dev(col)
    layer = CuGraphSAGEConv(cin, cout, root_weight=root_weight, project=project).cuda().to(T)
    assert all(p.dtype == T for p in layer.parameters())
    xb, _ = random_rows(rng, (n_src, cin), name)
    x = dev16(xb, name).requires_grad_(True)
    out = layer(x, rp, ci, 20)
    assert out.shape == (n_dst, cout) and out.dtype == T
    with torch.no_grad():
        h = layer.pre_lin(x).relu() if project else x
        cat_bits = round_bits(ref_forward(row_ptr, col, widen(bits(h), name), "mean"), name)
        cat = dev16(cat_bits, name)
        cat = cat if root_weight else cat[:, :cin]
        want = layer.lin(cat)
        scale = cat.float().abs() @ layer.lin.weight.float().abs().t() + layer.lin.bias.float().abs()
    rtol = 4 * torch.finfo(T).eps
    excess = (out.detach().float() - want.float()).abs() - rtol * scale
    assert bool((excess <= 0).all()), "max excess %g" % float(excess.max())
    out.float().square().sum().backward()
    params = dict(layer.named_parameters())
    assert "lin.weight" in params and (("pre_lin.weight" in params) == project)
    for pname, p in params.items():
        assert p.grad is not None and p.grad.dtype == T and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, pname
    assert x.grad is not None and x.grad.dtype == T and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0


# ---------------------------------------------------------------- 7 autocast end to end
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


def test_homo_gnn_model_trains_under_bf16_autocast(gpu_env):
    """the recipe of test_sage_agg_gpu.py::test_homo_gnn_model_trains_end_to_end (same graph, seeds, 40 steps, same
    criteria), with the forward and the loss under torch.autocast(bfloat16): layer 0 aggregates the fp32 features, its
    Linear returns bf16, and layer 1's agg_concat runs on bf16 rows (asserted with a forward hook)."""
    import torch
    import torch.nn.functional as Fn
    import wholegraph_amd.torch as wgth
    torch.manual_seed(1)
    rng = np.random.default_rng(2)
    n, k, dim = 4000, 4, 32
    row_ptr, col, labels_np = _planted_partition(n, k, rng)
    centres = rng.standard_normal((k, dim)).astype(F32)
    feats = (0.5 * centres[labels_np] + rng.standard_normal((n, dim)).astype(F32)).astype(F32)
    wrow, wcol = _wm_array(gpu_env, row_ptr), _wm_array(gpu_env, col)
    g = wgth.GraphStructure()
    g.set_csr_graph(wrow, wcol)
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [n, dim])
    emb.get_embedding_tensor().get_local_tensor()[0].copy_(torch.from_numpy(feats).cuda())
    wm_opt = wgth.create_wholememory_optimizer(emb, "adam", {})
    torch.cuda.synchronize()
    before = emb.get_embedding_tensor().get_local_tensor()[0].clone()

    wgth.set_framework("cugraph")
    args = types.SimpleNamespace(model="sage", hiddensize=64, layernum=2, classnum=k, dropout=0.1, neighbors="10,10",
                                 inferencesample="10,10", heads=1)
    model = wgth.HomoGNNModel(g, emb, args).cuda()
    seen = {0: [], 1: []}
    for i in (0, 1):
        model.gnn_layers[i].register_forward_pre_hook(lambda mod, inp, i=i: seen[i].append(inp[0].dtype))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    labels = torch.from_numpy(labels_np).cuda()
    losses = []
    model.train()
    for step in range(40):
        ids = torch.from_numpy(rng.choice(n, 256, replace=False).astype(np.int64)).cuda()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(ids)
            assert logits.shape == (256, k)
            loss = Fn.cross_entropy(logits, labels[ids])
        opt.zero_grad()
        loss.backward()
        opt.step()
        wm_opt.step(0.01)
        losses.append(float(loss.detach()))
    # the layers have no pre_lin: a layer's input is its agg_concat's input
    assert len(seen[1]) == 40 and set(seen[1]) == {torch.bfloat16}, "layer 1 did not aggregate bf16 rows"
    assert set(seen[0]) == {torch.float32}
    assert all(p.dtype == torch.float32 and p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print("autocast losses: first five %.4f, last five %.4f" % (first, last))
    assert np.isfinite(losses).all()
    assert last < 0.6 * first, "loss %.3f -> %.3f" % (first, last)
    after = emb.get_embedding_tensor().get_local_tensor()[0]
    changed = (after != before).any(dim=1)
    assert changed.float().mean() > 0.2, "gradients did not reach the WholeMemory embedding"
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ids = torch.arange(0, n, 4, device="cuda")
        acc = (model(ids).argmax(1) == labels[ids]).float().mean()
    print("autocast eval accuracy %.4f, embedding rows changed %.3f" % (float(acc), float(changed.float().mean())))
    assert acc > 0.7
    wgth.destroy_wholememory_optimizer(wm_opt)
    wgth.destroy_embedding(emb)
    wgth.destroy_wholememory_tensor(wrow)
    wgth.destroy_wholememory_tensor(wcol)


# ---------------------------------------------------------------- 8 the GAT layer under autocast (its op stays fp32)
@pytest.mark.parametrize("name", DTYPES)
def test_gat_conv_under_autocast(gpu_env, name):
    import torch
    from wholegraph_amd.torch.cugraphops.gat_conv import CuGraphGATConv
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n
    T = tdtype(name)
    torch.manual_seed(3)
    rng = np.random.default_rng(31)
    n_dst, n_src, cin, cout, heads = 60, 200, 24, 8, 2
    row_ptr, col = block(rng, n_dst, n_src, 12)
    rp, ci = dev(row_ptr), dev(col)
    layer = CuGraphGATConv(cin, cout, heads=heads).cuda()
    x = dev(rng.standard_normal((n_src, cin)).astype(F32)).requires_grad_(True)
    with torch.autocast("cuda", dtype=T):
        h = layer.lin(x)
        assert h.dtype == T
        op_out = mha_gat_n2n(h, layer.att, rp, ci, heads)
        assert op_out.dtype == torch.float32 and op_out.shape == (n_dst, heads * cout)
        out = layer(x, rp, ci, 12)
        assert out.dtype == torch.float32
        loss = out.square().sum()
    loss.backward()
    for p in (layer.lin.weight, layer.att):
        assert p.grad is not None and p.grad.dtype == torch.float32
        assert torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().sum() > 0
    # the op inside autocast is the fp32 op on the widened h
    with torch.no_grad():
        ref = mha_gat_n2n(h.detach().float(), layer.att, rp, ci, heads)
    assert torch.equal(op_out.detach(), ref)
    # outside autocast nothing changes: a 16-bit h is rejected
    with pytest.raises(TypeError, match="float32"):
        mha_gat_n2n(h.detach(), layer.att, rp, ci, heads)
