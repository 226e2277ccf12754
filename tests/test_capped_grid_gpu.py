"""Every row-kernel family of rows.hip under a workgroup cap (gather_sms / scatter_sms), against the CPU oracle, bit for bit.

Without a cap a launch is in order: one tile per wave, so `for (tile = wave; tile < tiles; tile += n_waves)` runs once, the
LDS-staged kernels get tiles of exactly one chunk, and power-of-two rows from 512 B up go to rows_batch_kernel. A caller who
passes gather_sms (a reference API parameter and a keyword of create_embedding) gets the persistent launch instead: waves
loop over many tiles, the staged kernels walk several R-row chunks inside a 64-row tile (the r0 loop, chunk_mask << r0, the
wave's LDS region reused behind the wave barrier), and those power-of-two rows are served by rows_copy16_fast_kernel. No
other test passes a cap.

Caps 1 and 3 (3 workgroups = 12 waves, which does not divide the tile counts), n = 5 (less than a tile: most waves idle),
64 (exactly one 64-row tile) and 2597 (41 tiles of 64 rows, the last one ragged: every wave loops at least three times),
int32 and int64 ids, duplicates for gather and unique ids for scatter, negative ids in the second half only (tiles with and
without a skipped entry), sentinel-filled outputs. One shape per kernel family and per chunk geometry; each case asserts
through the kernel's name that the intended family served the call."""
import ctypes as C

import numpy as np
import pytest

import _cast_values as cv
import oracle

pytestmark = pytest.mark.gpu

N_ROWS = 3001
CAPS = (1, 3)
BATCHES = (5, 64, 2597)
ID_DT = {"i32": np.int32, "i64": np.int64}

# name: (op, table dtype, plain dtype, dim, table stride, plain stride, kernel, template arguments that must match)
#   template arguments: {position: text} in the demangled name, e.g. rows_copy16_fast_kernel<IdxT, GATHER, RPS, HAS_MAP>
# rows_staged_*<IdxT, kStageIters>: 5 = chunks of up to 5 KiB, 10 = up to 10 KiB; R = rows per chunk, 64 / R chunks per tile
SHAPES = {
    # rows_copy_kernel<IdxT, VB, GATHER>
    "copy_12B":             ("gather", "f32", "f32", 3, 3, 3, "rows_copy_kernel", {1: "4"}),
    "copy_12B_s":           ("scatter", "f32", "f32", 3, 3, 3, "rows_copy_kernel", {1: "4"}),
    "copy_128B_out33":      ("gather", "f32", "f32", 32, 32, 33, "rows_copy_kernel", {1: "4"}),
    "copy_128B_in33_s":     ("scatter", "f32", "f32", 32, 32, 33, "rows_copy_kernel", {1: "4"}),
    "copy_1B":              ("gather", "i8", "i8", 1, 1, 1, "rows_copy_kernel", {1: "1"}),
    "copy_1B_s":            ("scatter", "i8", "i8", 1, 1, 1, "rows_copy_kernel", {1: "1"}),
    # rows_copy16_fast_kernel<IdxT, GATHER, RPS, HAS_MAP>: 512 B = two rows per step (the C2 shape), above = one row per step
    "fast_512B":            ("gather", "f32", "f32", 128, 128, 128, "rows_copy16_fast_kernel", {2: "2"}),
    "fast_512B_s":          ("scatter", "f32", "f32", 128, 128, 128, "rows_copy16_fast_kernel", {2: "2"}),
    "fast_1KiB":            ("gather", "f32", "f32", 256, 256, 256, "rows_copy16_fast_kernel", {2: "1"}),
    "fast_1KiB_s":          ("scatter", "f32", "f32", 256, 256, 256, "rows_copy16_fast_kernel", {2: "1"}),
    "fast_2KiB":            ("gather", "f32", "f32", 512, 512, 512, "rows_copy16_fast_kernel", {2: "1"}),   # two 1 KiB chunks per row
    "fast_2KiB_s":          ("scatter", "f32", "f32", 512, 512, 512, "rows_copy16_fast_kernel", {2: "1"}),
    # rows_flat_kernel<IdxT, GATHER, HAS_MAP>
    "flat_800B":            ("gather", "f32", "f32", 200, 200, 200, "rows_flat_kernel", {1: "true"}),
    "flat_5200B_s":         ("scatter", "f32", "f32", 1300, 1300, 1300, "rows_flat_kernel", {1: "false"}),  # above the staged kernels' 5120 B
    "flat_400B_in101_s":    ("scatter", "f32", "f32", 100, 100, 101, "rows_flat_kernel", {1: "false"}),     # strided input
    # rows_staged_gather_kernel / rows_staged_scatter_kernel, 5 slots
    "staged_132B":          ("gather", "f32", "f32", 33, 36, 33, "rows_staged_gather_kernel", {1: "5"}),    # R = 32
    "staged_144B_s":        ("scatter", "f32", "f32", 36, 36, 36, "rows_staged_scatter_kernel", {1: "5"}),  # R = 32 (132 B scatters are not staged)
    "staged_400B":          ("gather", "f32", "f32", 100, 100, 100, "rows_staged_gather_kernel", {1: "5"}),  # R = 8
    "staged_400B_s":        ("scatter", "f32", "f32", 100, 100, 100, "rows_staged_scatter_kernel", {1: "5"}),
    "staged_1204B":         ("gather", "f16", "f16", 602, 608, 602, "rows_staged_gather_kernel", {1: "5"}),  # R = 4
    "staged_1204B_s":       ("scatter", "f16", "f16", 602, 608, 602, "rows_staged_scatter_kernel", {1: "5"}),
    "staged_2408B":         ("gather", "f32", "f32", 602, 604, 602, "rows_staged_gather_kernel", {1: "5"}),  # R = 2
    "staged_2408B_s":       ("scatter", "f32", "f32", 602, 604, 602, "rows_staged_scatter_kernel", {1: "5"}),
    # ... 10 slots
    "staged_4120B":         ("gather", "f32", "f32", 1030, 1032, 1030, "rows_staged_gather_kernel", {1: "10"}),  # R = 2
    "staged_4120B_s":       ("scatter", "f32", "f32", 1030, 1032, 1030, "rows_staged_scatter_kernel", {1: "10"}),
    # rows_convert_kernel<TabT, PlainT, IdxT, V, GATHER>
    "cast_f16_f32_128":     ("gather", "f16", "f32", 128, 128, 128, "rows_convert_kernel", {3: "4"}),
    "cast_f16_f32_33":      ("gather", "f16", "f32", 33, 33, 33, "rows_convert_kernel", {3: "1"}),
    "cast_f32_bf16_128":    ("gather", "f32", "bf16", 128, 128, 128, "rows_convert_kernel", {3: "4"}),
    "cast_f32_bf16_33":     ("gather", "f32", "bf16", 33, 33, 33, "rows_convert_kernel", {3: "1"}),
    "cast_f16_f32_128_s":   ("scatter", "f32", "f16", 128, 128, 128, "rows_convert_kernel", {3: "4"}),   # plain f16 -> f32 table
    "cast_f16_f32_33_s":    ("scatter", "f32", "f16", 33, 33, 33, "rows_convert_kernel", {3: "1"}),
    "cast_f32_bf16_128_s":  ("scatter", "bf16", "f32", 128, 128, 128, "rows_convert_kernel", {3: "4"}),  # plain f32 -> bf16 table
    "cast_f32_bf16_33_s":   ("scatter", "bf16", "f32", 33, 33, 33, "rows_convert_kernel", {3: "1"}),
}
# also on a distributed table (the cap travels through gather_distributed_rows) and with the persistent launch at its own grid
# size (WM_ROWS_INORDER=0, no cap). With one rank a continuous, a chunked and a distributed table all reach the kernels as a
# flat reference: the memory types differ in the host code in front of the launch, not in how a row's owner is found. Owner
# resolution under a cap is what test_capped_grid_chunked_reference_of_several_ranks is for.
EXTRA = ["fast_512B", "fast_512B_s", "staged_400B", "staged_400B_s"]
CASTS = ["cast_f16_f32_128", "cast_f32_bf16_33", "cast_f16_f32_33_s", "cast_f32_bf16_128_s"]


def _values(name, shape, seed):
    """random elements of dtype `name` (carrier array): small integers and halves — exact in every float type here, so that
    a cast case checks the launch and not the rounding (tests/test_cast_values_gpu.py does that)"""
    rng = np.random.default_rng(seed)
    if name == "i8":
        return rng.integers(-128, 127, shape, dtype=np.int8, endpoint=True)
    v = rng.integers(-240, 240, shape).astype(np.float32) / 2
    if name == "bf16":
        return (v.view(np.uint32) >> 16).astype(np.uint16)      # exact: |2 v| < 2^8
    return v.astype(cv.CARRIER[name])


def _assert_served_by(kernel, targs, what):
    from wholegraph_amd import binding as wmb
    name = wmb.lib().wholememory_ext_last_rows_kernel().decode()
    family, args = cv.rows_kernel(name)
    assert family == kernel, "%s: served by %r, not by %s" % (what, name, kernel)
    for pos, text in targs.items():
        assert args[pos] == text, "%s: template argument %d of %r is not %s" % (what, pos, name, text)


def _ids(rng, n, idt, unique):
    if unique:
        idx = rng.permutation(N_ROWS)[:n].astype(ID_DT[idt])
    else:
        idx = rng.integers(0, N_ROWS, n).astype(ID_DT[idt])
        idx[: min(n, 7)] = idx[0]                                   # duplicates, next to each other and apart
        idx[n // 3] = idx[0]
    idx[n // 2 + 1::29] = -1                                        # skipped entries: second half only
    assert (idx[: n // 2 + 1] >= 0).all() and (idx < 0).any()
    return idx


class Table:
    """a WholeMemory table [N_ROWS, stride] of random values and its oracle twin; `view` is the [N_ROWS, dim] part"""

    def __init__(self, comm, mt, name, dim, stride):
        import wholegraph_amd.torch as wgth
        self.name, self.dim, self.stride = name, dim, stride
        self.root = wgth.create_wholememory_tensor(comm, mt, "cuda", [N_ROWS, stride], cv.torch_dtype(name), [stride, 1])
        self.view = self.root.get_sub_tensor([0, 0], [N_ROWS, dim]) if dim != stride else self.root
        self.local, start = self.root.get_local_tensor(host_view=False)
        assert start == 0 and tuple(self.local.shape) == (N_ROWS, stride)
        self.fill(_values(name, (N_ROWS, stride), 5))

    def fill(self, full):
        import torch
        self.full = full
        self.local.copy_(cv.to_torch(full, self.name).cuda())
        torch.cuda.synchronize()

    def oracle_table(self):
        return oracle.ShardedTable([self.full], np.array([0, N_ROWS], dtype=np.uint64), self.dim, self.stride, 0,
                                   cv.ORACLE_DT[self.name])

    def destroy(self):
        import wholegraph_amd.torch as wgth
        if self.view is not self.root:
            wgth.destroy_wholememory_tensor(self.view)
        wgth.destroy_wholememory_tensor(self.root)


def run_gather(tab, pdt, pstride, n, idt, cap, kernel, targs, what):
    import torch
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor, get_wholegraph_env_fns, get_stream
    rng = np.random.default_rng(n * 7 + (cap if cap > 0 else 0))
    idx = _ids(rng, n, idt, unique=False)
    want = np.full((n, pstride), cv.sentinel(pdt), dtype=cv.CARRIER[pdt])
    out_t = cv.to_torch(want.copy(), pdt).cuda()
    wi = wrap_torch_tensor(torch.from_numpy(idx).cuda())
    wo = wrap_torch_tensor(out_t[:, :tab.dim] if pstride != tab.dim else out_t)
    wmb.check(wmb.lib().wholememory_gather(tab.view.wmb_tensor, wi.handle, wo.handle, get_wholegraph_env_fns(),
                                           C.c_void_p(get_stream()), cap))
    torch.cuda.synchronize()
    _assert_served_by(kernel, targs, what)
    oracle.gather(tab.oracle_table(), idx, want, dim=tab.dim, out_stride=pstride, out_dt=cv.ORACLE_DT[pdt])
    got = cv.from_torch(out_t, pdt)
    differ = cv.bits_of(got) != cv.bits_of(want)
    assert not differ.any(), "%s: %d elements in %d of %d output rows differ from the oracle, first row %d (id %d)" % (
        what, differ.sum(), differ.any(axis=1).sum(), n, np.argwhere(differ)[0][0], idx[np.argwhere(differ)[0][0]])


def run_scatter(tab, pdt, pstride, n, idt, cap, kernel, targs, what):
    import torch
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor, get_wholegraph_env_fns, get_stream
    rng = np.random.default_rng(n * 11 + (cap if cap > 0 else 0))
    idx = _ids(rng, n, idt, unique=True)
    tab.fill(np.full((N_ROWS, tab.stride), cv.sentinel(tab.name), dtype=cv.CARRIER[tab.name]))
    rows = _values(pdt, (n, pstride), n + 1)
    rows_t = cv.to_torch(rows, pdt).cuda()
    ws = wrap_torch_tensor(rows_t[:, :tab.dim] if pstride != tab.dim else rows_t)
    wi = wrap_torch_tensor(torch.from_numpy(idx).cuda())
    wmb.check(wmb.lib().wholememory_scatter(ws.handle, wi.handle, tab.view.wmb_tensor, get_wholegraph_env_fns(),
                                            C.c_void_p(get_stream()), cap))
    torch.cuda.synchronize()
    _assert_served_by(kernel, targs, what)
    ref = oracle.ShardedTable([tab.full.copy()], np.array([0, N_ROWS], dtype=np.uint64), tab.dim, tab.stride, 0,
                              cv.ORACLE_DT[tab.name])
    oracle.scatter(rows, idx, ref, dim=tab.dim, in_stride=pstride, in_dt=cv.ORACLE_DT[pdt])
    got, want = cv.from_torch(tab.local, tab.name), ref.shards[0]
    differ = cv.bits_of(got) != cv.bits_of(want)
    assert not differ.any(), "%s: %d elements in %d table rows differ from the oracle (untouched rows and pad columns included)" % (
        what, differ.sum(), differ.any(axis=1).sum())


def run_shape(comm, mt, shape, caps):
    op, tdt, pdt, dim, tstride, pstride, kernel, targs = SHAPES[shape]
    tab = Table(comm, mt, tdt, dim, tstride)
    try:
        for cap in caps:
            for n in BATCHES:
                for idt in ("i32", "i64"):
                    what = "%s %s on a %s table, cap %d, n %d, %s ids" % (op, shape, mt, cap, n, idt)
                    (run_gather if op == "gather" else run_scatter)(tab, pdt, pstride, n, idt, cap, kernel, targs, what)
    finally:
        tab.destroy()


@pytest.mark.parametrize("mt", ["continuous", "chunked"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_capped_grid(gpu_env, shape, mt):
    run_shape(gpu_env, mt, shape, CAPS)


@pytest.mark.parametrize("shape", EXTRA)
def test_capped_grid_distributed(gpu_env, shape):
    run_shape(gpu_env, "distributed", shape, CAPS)


@pytest.mark.parametrize("world", [2, 3])
def test_capped_grid_chunked_reference_of_several_ranks(wm_lib, world):
    """A table of one rank reaches the kernels as a flat reference whatever its memory type, so nothing above resolves an
    owner. Here `world` processes share the GPU (tests/_dist_worker.py: scenario_capped_rows): a device CHUNKED table mapped
    across them is a real chunked reference, and the capped and WM_ROWS_INORDER=0 launches of the 512 B and 400 B shapes
    find each row's owner from the tables passed by value and, with WM_ROWS_OWNERS_BY_VALUE=0, from the reference's device
    arrays — the multiply-high for equal chunks and the search over rank offsets for a custom partition."""
    from test_distributed_cpu import run_world
    run_world(world, "hip", {"WM_TEST_ONLY": "capped_rows"})


@pytest.mark.parametrize("shape", EXTRA + CASTS)
def test_persistent_launch_without_a_cap(gpu_env, knobs, shape):
    """WM_ROWS_INORDER=0: the persistent launch at its own grid size. At these sizes the grid covers the tiles, so this
    checks the launch shape and the staged kernels' 64-row tiles, not the loop."""
    knobs.set("WM_ROWS_INORDER", "0")
    run_shape(gpu_env, "chunked", shape, (-1,))


@pytest.mark.parametrize("cached", [False, True], ids=["uncached", "cached"])
def test_embedding_gather_sms(gpu_env, cached):
    """create_embedding(..., gather_sms=2): the cap reaches the row kernels from the embedding, directly and through
    gather_cached behind a 20 % read-only device cache (there the hits and the misses are one capped row gather each; the
    last one launched is named). Without the cap these 512 B rows would be served by rows_batch_kernel."""
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding as wmb
    n_rows, dim = 20011, 128
    policy = None
    if cached:
        policy = wgth.create_wholememory_cache_policy(gpu_env, memory_type="chunked", memory_location="cuda",
                                                      access_type="readonly", ratio=0.2)
    emb = wgth.create_embedding(gpu_env, "chunked", "cuda", torch.float32, [n_rows, dim], cache_policy=policy, gather_sms=2)
    try:
        full = _values("f32", (n_rows, dim), 9)
        local, _ = emb.get_embedding_tensor().get_local_tensor()
        local.copy_(torch.from_numpy(full).cuda())
        torch.cuda.synchronize()
        tab = oracle.ShardedTable.from_full(full, 1)
        rng = np.random.default_rng(2)
        for b, n in enumerate((2597, 64, 2597, 5)):       # (the second large batch finds rows of the first in the cache)
            idx = ((rng.zipf(1.3, n).astype(np.uint64) * np.uint64(2654435761)) % np.uint64(n_rows)).astype(np.int64)
            idx[n // 2 + 1::29] = -1
            out = torch.full((n, dim), -7.0, device="cuda")
            emb.gather(torch.from_numpy(idx).cuda(), out=out)
            torch.cuda.synchronize()
            _assert_served_by("rows_copy16_fast_kernel", {2: "2"}, "embedding gather, batch %d" % b)
            want = np.full((n, dim), -7.0, dtype=np.float32)
            oracle.gather(tab, idx, want)
            assert out.cpu().numpy().tobytes() == want.tobytes(), "batch %d" % b
        if cached:
            v = [C.c_int64() for _ in range(5)]   # slots, occupied, dirty, hits, lookups
            wmb.check(wmb.lib().wholememory_ext_embedding_cache_info(emb.wmb_embedding, *[C.byref(x) for x in v]))
            assert v[1].value > 0 and v[3].value > 0, "no row was served from the cache: %s" % [x.value for x in v]
    finally:
        wgth.destroy_embedding(emb)
        if policy is not None:
            wgth.destroy_wholememory_cache_policy(policy)
