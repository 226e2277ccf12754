"""8-bit row-quantized tables on the MI355X (wholegraph_amd/torch/quantized.py -> csrc/quantized.cpp ->
csrc/kernels/qrows.hip; header section 2i).

Every comparison is bitwise (torch.equal / np.array_equal on integer views) against the numpy restatement of the row format
in tests/test_qrows_surface.py (quantize_ref / dequantize_ref: float32 operations, each rounded on its own), rounded once
more by numpy / torch on the host for the 16-bit outputs. The reference of a (rows, dim) pair is computed once and shared."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_qrows_surface import dequantize_ref, quantize_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
DIMS = [1, 3, 4, 11, 32, 127, 128, 129, 513]
OUT_DTYPES = ["float32", "float16", "bfloat16"]
N_ROWS, N_IDS = 1003, 2000
SENTINEL = -7.0


def mixed_rows(rng, n, dim):
    """rows of four kinds in turn: magnitudes spread over 2^+-12 binades; constant rows (zero, and values of either sign);
    N(0, 1) rows with one outlier of 1e6; rows offset by 1000"""
    x = np.empty((n, dim), F32)
    k = np.arange(n) % 4
    x[k == 0] = (rng.standard_normal((int((k == 0).sum()), dim)) * np.exp2(rng.integers(-12, 13, (int((k == 0).sum()), dim))))
    consts = rng.standard_normal(int((k == 1).sum())) * 100.0
    consts[::5] = 0.0
    x[k == 1] = consts.astype(F32)[:, None]
    outl = rng.standard_normal((int((k == 2).sum()), dim))
    outl[np.arange(len(outl)), rng.integers(0, dim, len(outl))] = 1e6
    x[k == 2] = outl
    x[k == 3] = 1000.0 + rng.standard_normal((int((k == 3).sum()), dim))
    return x


@functools.lru_cache(maxsize=None)
def reference(n, dim):
    """(x, raw, y): values, their quantized rows (uint8) and what those dequantize to (float32); read-only"""
    x = mixed_rows(np.random.default_rng(1000 * dim + n), n, dim)
    raw = quantize_ref(x)
    y = dequantize_ref(raw, dim)
    for a in (x, raw, y):
        a.setflags(write=False)
    return x, raw, y


@functools.lru_cache(maxsize=None)
def lookup_ids(n_rows, n_ids):
    """ids with duplicates, the first and the last row, and about 5 % negatives"""
    rng = np.random.default_rng(n_rows + n_ids)
    ids = rng.integers(0, n_rows, n_ids)
    ids[:3] = [0, n_rows - 1, 0]
    ids[rng.random(n_ids) < 0.05] = -1
    ids[7] = -1
    ids.setflags(write=False)
    return ids


def narrowed(y, dtype):
    """float32 numpy -> host torch tensor of `dtype` (round to nearest even, once)"""
    import torch
    return torch.from_numpy(np.array(y, F32)).to(getattr(torch, dtype))


def same_bits(a, b):
    import torch
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(view), b.view(view))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared references are read-only)


def all_rows(n):
    import torch
    return torch.arange(n, dtype=torch.int64, device="cuda")


def make_table(comm, mt, loc, x, **kw):
    """a quantized table filled with the rows x (numpy float32) through its own scatter"""
    import torch
    import wholegraph_amd.torch as wgth
    t = wgth.create_quantized_tensor(comm, mt, loc, list(x.shape), **kw)
    t.scatter(dev(x), all_rows(x.shape[0]))
    torch.cuda.synchronize()
    return t


def destroy(t):
    import wholegraph_amd.torch as wgth
    wgth.destroy_wholememory_tensor(t.storage)


def raw_of(t):
    """the table's rows as the int8 gather returns them: [N, row_bytes]"""
    return t.storage.gather(all_rows(t.shape[0]))


def gather_into(t, ids, out, sms=-1):
    """the C entry point, writing into `out` (any view with unit inner stride)"""
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import get_stream, get_wholegraph_env_fns, wrap_torch_tensor
    wmb.check(wmb.lib().wholememory_ext_gather_dequantize(
        t.storage.wmb_tensor, t.dim_, wrap_torch_tensor(ids) if ids is not None else None, wrap_torch_tensor(out),
        get_wholegraph_env_fns(), C.c_void_p(get_stream()), sms))


def check_gather(t, y, ids_np, id_dtype=np.int64, dtypes=OUT_DTYPES, fused=True, pad=3):
    """gather of every output dtype into a sentinel-filled, padded buffer == numpy; returns the float32 result"""
    import torch
    from wholegraph_amd.torch import quantized
    ids = dev(ids_np.astype(id_dtype))
    dim, n = t.dim_, len(ids_np)
    skip = ids_np < 0
    first = None
    for dtype in dtypes:
        tdt = getattr(torch, dtype)
        buf = torch.full((n, dim + pad), SENTINEL, dtype=tdt, device="cuda")
        before = quantized.calls()
        gather_into(t, ids, buf[:, :dim])
        assert quantized.calls() == before + (1 if fused and n > 0 else 0)
        torch.cuda.synchronize()
        want = narrowed(np.where(skip[:, None], F32(SENTINEL), y[np.maximum(ids_np, 0)]), dtype)
        assert same_bits(buf[:, :dim], want), (dtype, dim)
        assert bool((buf[:, dim:] == SENTINEL).all()), "columns past dim were written"
        got = t.gather(ids, force_dtype=tdt)     # the Python method: rows of negative ids are whatever torch.empty left
        assert got.dtype == tdt and got.shape == (n, dim)
        assert same_bits(got[dev(~skip)], want[torch.from_numpy(~skip)])
        first = buf[:, :dim].contiguous() if first is None else first
    return first


# ---------------------------------------------------------------- 1 quantize_rows / dequantize_rows round trip
@pytest.mark.parametrize("dim", DIMS)
def test_round_trip_of_local_rows(gpu_env, dim):
    import torch
    import wholegraph_amd.torch as wgth
    x, raw, y = reference(257, dim)
    got_raw = wgth.quantize_rows(dev(x))
    assert got_raw.dtype == torch.int8 and got_raw.shape == (257, wgth.quantized_row_bytes(dim))
    assert np.array_equal(got_raw.cpu().numpy().view(np.uint8), raw)   # codes, the zero padding and the trailer
    for dtype in OUT_DTYPES:
        got = wgth.dequantize_rows(got_raw, dim, getattr(torch, dtype))
        assert same_bits(got, narrowed(y, dtype)), dtype
    # 16-bit values are widened first
    h = torch.from_numpy(np.array(x)).clamp(-6e4, 6e4).to(torch.float16)
    assert torch.equal(wgth.quantize_rows(h.cuda()).cpu(), torch.from_numpy(quantize_ref(h.float().numpy()).view(np.int8)))


# ---------------------------------------------------------------- 2 the fused gather
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("mt", ["continuous", "chunked"])
def test_fused_gather(gpu_env, mt, dim):
    import torch
    import wholegraph_amd.torch as wgth
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, mt, "cuda", x)
    assert t.shape == (N_ROWS, dim) and t.storage.shape == (N_ROWS, wgth.quantized_row_bytes(dim))
    assert t.storage.stride()[0] == (wgth.quantized_row_bytes(dim) + 15) // 16 * 16
    assert np.array_equal(raw_of(t).cpu().numpy().view(np.uint8), raw)
    ids_np = lookup_ids(N_ROWS, N_IDS)
    a = check_gather(t, y, ids_np, np.int64)
    b = check_gather(t, y, ids_np, np.int32, dtypes=["float32"])
    assert same_bits(a, b)
    # ... and equals the two-op composition on the rows that were asked for
    ids = dev(ids_np)
    two = wgth.dequantize_rows(t.storage.gather(ids), dim)
    keep = dev(ids_np >= 0)
    assert same_bits(a[keep], two[keep])
    destroy(t)


# ---------------------------------------------------------------- 3 row strides and views
@pytest.mark.parametrize("dim", [11, 128])
@pytest.mark.parametrize("row_align", [4, 16, 128])
def test_row_strides(gpu_env, dim, row_align):
    import wholegraph_amd.torch as wgth
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=row_align)
    rb = wgth.quantized_row_bytes(dim)
    assert t.storage.stride()[0] == (rb + row_align - 1) // row_align * row_align   # e.g. 20 bytes for dim 11, align 4
    assert np.array_equal(raw_of(t).cpu().numpy().view(np.uint8), raw)
    check_gather(t, y, lookup_ids(N_ROWS, N_IDS))
    destroy(t)


@pytest.mark.parametrize("dim,row_align", [(11, 4), (128, 16)])
def test_row_range_view_of_the_storage(gpu_env, dim, row_align):
    import torch
    import wholegraph_amd.torch as wgth
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=row_align)
    r0, r1 = 101, 901
    view = wgth.WholeMemoryQuantizedTensor(t.storage.get_sub_tensor([r0, 0], [r1, -1]), dim)
    assert view.shape == (r1 - r0, dim) and view.storage.storage_offset() == r0 * t.storage.stride()[0]
    ids_np = lookup_ids(r1 - r0, 700)
    check_gather(view, y[r0:r1], ids_np)
    # a scatter through the view lands in the table's rows r0 + id
    new = np.ascontiguousarray(x[::-1][:50])
    view.scatter(dev(new), torch.arange(50, device="cuda"))
    want = raw.copy()
    want[r0:r0 + 50] = quantize_ref(new)
    assert np.array_equal(raw_of(t).cpu().numpy().view(np.uint8), want)
    destroy(t)


# ---------------------------------------------------------------- 4 sizes and the capped grid
def test_sizes_and_capped_grids(gpu_env):
    """The gather's grid is min(ceil(n / 256), 32 * CUs [, gather_sms]) workgroups of 4 waves, a wave takes 64 consecutive ids
    per pass and strides by the number of waves. So one pass of the default grid covers 32 * CUs * 256 ids — anything beyond
    that makes every wave of the first workgroups loop — and one pass of gather_sms = 1 covers 256."""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import quantized
    dim = 4
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cuda", x)
    for n in (0, 1):
        before = quantized.calls()
        got = t.gather(torch.full((n,), 5, dtype=torch.int64, device="cuda"))
        assert got.shape == (n, dim) and quantized.calls() == before + n      # (n = 0: success without a launch)
        assert same_bits(got, torch.from_numpy(y[[5] * n].reshape(n, dim)))
    one_pass = 32 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    n = one_pass + 64 * 3 + 13
    ids_np = np.random.default_rng(3).integers(0, N_ROWS, n)
    ids_np[::101] = -1
    buf = torch.full((n, dim), SENTINEL, device="cuda")
    gather_into(t, dev(ids_np), buf)
    want = np.where((ids_np < 0)[:, None], F32(SENTINEL), y[np.maximum(ids_np, 0)])
    assert same_bits(buf, torch.from_numpy(want))
    # gather_sms = 1: one workgroup walks 2000 ids in 8 passes; a wider row too
    for d in (4, 129):
        x, raw, y = reference(N_ROWS, d)
        td = t if d == dim else make_table(gpu_env, "chunked", "cuda", x)
        ids_np = lookup_ids(N_ROWS, N_IDS)
        buf = torch.full((N_IDS, d), SENTINEL, device="cuda")
        gather_into(td, dev(ids_np), buf, sms=1)
        want = np.where((ids_np < 0)[:, None], F32(SENTINEL), y[np.maximum(ids_np, 0)])
        assert same_bits(buf, torch.from_numpy(want))
        if td is not t:
            destroy(td)
    destroy(t)


# ---------------------------------------------------------------- 5 tables in host memory
@pytest.mark.parametrize("dim", [64, 129])
def test_host_located_table(gpu_env, dim):
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cpu", x)
    assert np.array_equal(raw_of(t).cpu().numpy().view(np.uint8), raw)
    check_gather(t, y, lookup_ids(N_ROWS, N_IDS))
    destroy(t)


def test_large_batches_from_a_host_table_take_the_sorted_raw_gather(gpu_env, knobs):
    """from WM_HOST_SORTED_MIN ids on (2^19 by default; lowered here) the raw rows of a host table are gathered in ascending
    row order and dequantized locally: the same values, and the table-reading kernel's counter does not move"""
    from wholegraph_amd import binding as wmb
    dim = 64
    x, raw, y = reference(N_ROWS, dim)
    t = make_table(gpu_env, "chunked", "cpu", x)
    ids_np = lookup_ids(N_ROWS, N_IDS)
    knobs.set("WM_HOST_SORTED_MIN", N_IDS)
    sorted_before = wmb.lib().wholememory_ext_host_sorted_gathers()
    a = check_gather(t, y, ids_np, fused=False)
    assert wmb.lib().wholememory_ext_host_sorted_gathers() > sorted_before
    knobs.set("WM_HOST_SORTED_MIN", N_IDS + 1)
    assert same_bits(a, check_gather(t, y, ids_np, dtypes=["float32"], fused=True))
    destroy(t)


# ---------------------------------------------------------------- 6 the exchange route
@pytest.mark.parametrize("dim", [11, 128])
def test_distributed_table_takes_the_exchange_route(gpu_env, dim):
    """world size 1: the raw rows move through the exchange, the kernels work on the local side; same bytes, same values,
    and the fused-route counter does not move"""
    from wholegraph_amd.torch import quantized
    x, raw, y = reference(N_ROWS, dim)
    before = quantized.calls()
    t = make_table(gpu_env, "distributed", "cuda", x)
    assert np.array_equal(raw_of(t).cpu().numpy().view(np.uint8), raw)
    ids_np = lookup_ids(N_ROWS, N_IDS)
    a = check_gather(t, y, ids_np, fused=False)
    check_gather(t, y, ids_np, np.int32, dtypes=["float32"], fused=False)
    assert quantized.calls() == before
    m = make_table(gpu_env, "chunked", "cuda", x)
    assert same_bits(raw_of(t), raw_of(m))
    assert same_bits(a, check_gather(m, y, ids_np, dtypes=["float32"]))
    destroy(t)
    destroy(m)


# ---------------------------------------------------------------- 7 the fused scatter
@pytest.mark.parametrize("dim", [3, 11, 128, 513])
@pytest.mark.parametrize("mt", ["continuous", "chunked"])
def test_fused_scatter(gpu_env, mt, dim):
    """distinct ids (and negative ones) into a table whose every byte is 0x5a: the addressed rows equal quantize_rows + a raw
    scatter byte for byte, nothing else changes — the stride's padding bytes included"""
    import torch
    import wholegraph_amd.torch as wgth
    x, raw, y = reference(N_ROWS, dim)
    rb = wgth.quantized_row_bytes(dim)

    def padding(t):
        """(rows [N, row_bytes], the bytes between the rows [N - 1, stride - row_bytes]) of the table's memory"""
        local, start = t.storage.get_local_tensor()
        stride = local.stride(0)
        assert start == 0 and local.shape == (N_ROWS, rb) and stride % 64 == 0 and stride > rb
        return local, torch.as_strided(local, (N_ROWS - 1, stride), (stride, 1))[:, rb:]

    tables = []
    for _ in range(2):
        t = wgth.create_quantized_tensor(gpu_env, mt, "cuda", [N_ROWS, dim], row_align=64)
        for part in padding(t):
            part.fill_(0x5a)
        tables.append(t)
    fused, two_op = tables
    rng = np.random.default_rng(dim)
    ids_np = rng.permutation(N_ROWS)[:400]
    ids_np[::9] = -1
    rows = np.ascontiguousarray(x[rng.integers(0, N_ROWS, 400)])
    for idt in (np.int64, np.int32):
        ids = dev(ids_np.astype(idt))
        fused.scatter(dev(rows), ids)
        two_op.storage.scatter(wgth.quantize_rows(dev(rows)), ids)
        torch.cuda.synchronize()
        want = np.full((N_ROWS, rb), 0x5a, np.uint8)
        want[ids_np[ids_np >= 0]] = quantize_ref(rows)[ids_np >= 0]
        for t in tables:
            local, between = padding(t)
            assert np.array_equal(local.cpu().numpy().view(np.uint8), want)
            assert bool((between == 0x5a).all())
    for t in tables:
        destroy(t)


# ---------------------------------------------------------------- 8 two ranks sharing one device
def test_two_ranks_sharing_one_device(wm_lib):
    """a CHUNKED table whose halves live in two processes (peer rows through the hipIpc mapping, equal chunks and a custom
    partition) and a DISTRIBUTED one (the exchange route at world size 2), both ranks on cuda:0, collectives over gloo"""
    from test_distributed_cpu import free_port
    port = str(free_port())
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_qrows_worker.py"), str(r), "2", port], env=env,
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
