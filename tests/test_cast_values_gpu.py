"""Conversions of the row kernels (rows.hip: rows_convert_kernel, device_common.cuh: convert_elt) on the values where a
conversion goes wrong, against the CPU oracle, bit for bit.

The other GPU tests feed the casts small integers or randn * 100: nothing there is a round-to-nearest-even tie, a 16-bit
subnormal, an overflow to infinity, -0, inf or NaN, and no test runs a bf16 cast at all. Here (tests/_cast_values.py):
  * 16-bit sources (f16, bf16): all 65 536 bit patterns, so widening and 16 -> 16 casts are exhaustive;
  * f32 sources: every midpoint between neighbouring finite f16 / bf16 values with its two f32 neighbours, both signs, the
    overflow boundary, the tie to zero, f32 subnormals, +-0, +-inf, 2 k random values over eight magnitudes;
  * f64 sources: the f32 set widened, ties of f32 itself with their f64 neighbours, f32's overflow and underflow boundaries,
    +-1e300, and m (1 +- 2^-40) for every 16-bit tie m, where f64 -> f32 -> 16-bit (the reference's chain, which convert_elt
    promises) differs from one rounding;
  * NaNs: quiet and signalling, both signs. A NaN input must give a NaN (hardware and C disagree on payload bits); the
    count of NaN inputs is asserted. Every other element, skipped rows and pad columns included, is compared bit for bit;
  * the twelve integer pairs on both types' limits and their neighbours and 8 k random full-range values.
Each set is laid out as a table of width dim (64 / 66 / 65: 4-, 2- and 1-element vectors per lane) and every row is gathered
in a permuted order, with negative ids in the second half of the batch only (tiles with and without a skipped entry: the
kernel's straight-line and per-step paths), into a sentinel-filled output with a padded stride; then the same values are
scattered from a plain tensor of the source dtype into a zeroed table of the target dtype.
The three memory types of the float cases differ in the host code in front of the launch only: a table of one rank reaches the
kernels as a flat reference whichever it is."""
import ctypes as C

import numpy as np
import pytest

import _cast_values as cv
import oracle

pytestmark = pytest.mark.gpu

VEC_OF_DIM = {64: 4, 66: 2, 65: 1}
ID_DT = {"i32": np.int32, "i64": np.int64}


def _served_by():
    from wholegraph_amd import binding as wmb
    return wmb.lib().wholememory_ext_last_rows_kernel().decode()


def _assert_convert_kernel(name, vec, gather):
    """the call was served by rows_convert_kernel<TabT, PlainT, IdxT, V, GATHER> with V = vec"""
    family, args = cv.rows_kernel(name)
    assert family == "rows_convert_kernel", "not a converting launch: %r" % name
    assert args[3] == str(vec) and args[4] == ("true" if gather else "false"), name


def _ids(rng, n_rows, idt):
    """every row once, permuted; some negative ids in the second half only"""
    idx = rng.permutation(n_rows).astype(ID_DT[idt])
    idx[n_rows // 2 + 3::41] = -1
    return idx


def _compare(got, want, nan_in, dst, what):
    assert cv.isnan(got, dst)[nan_in].all(), "%s: a NaN input did not give a NaN" % what
    differ = (cv.bits_of(got) != cv.bits_of(want)) & ~nan_in
    if differ.any():
        r, c = np.argwhere(differ)[0]
        raise AssertionError("%s: %d of %d elements differ from the oracle, first at [%d, %d]: %#x, oracle %#x" % (
            what, differ.sum(), differ.size, r, c, cv.bits_of(got)[r, c], cv.bits_of(want)[r, c]))


def run_pair(comm, src, dst, dim, idt, mt, values, n_nan):
    import torch
    import wholegraph_amd.torch as wgth
    from wholegraph_amd import binding as wmb
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor, get_wholegraph_env_fns, get_stream
    table = cv.as_table(values, dim, src)
    n_rows, pad = table.shape[0], 4             # (a pad of 4 elements keeps the vector width that dim selects)
    nan_tab = cv.isnan(table, src) if n_nan else np.zeros(table.shape, dtype=bool)
    assert int(nan_tab.sum()) == n_nan
    rng = np.random.default_rng(17 + dim)
    env, stream = get_wholegraph_env_fns(), C.c_void_p(get_stream())

    # ---- gather: table of the source dtype -> sentinel-filled plain output of the target dtype, stride dim + pad
    root = wgth.create_wholememory_tensor(comm, mt, "cuda", [n_rows, dim], cv.torch_dtype(src), [dim, 1])
    local, start = root.get_local_tensor(host_view=False)
    assert start == 0 and tuple(local.shape) == (n_rows, dim)
    local.copy_(cv.to_torch(table, src).cuda())
    idx = _ids(rng, n_rows, idt)
    valid = idx >= 0
    assert valid[:n_rows // 2].all() and not valid[n_rows // 2:].all()
    want = np.full((n_rows, dim + pad), cv.sentinel(dst), dtype=cv.CARRIER[dst])
    out_t = cv.to_torch(want.copy(), dst).cuda()
    wi, wo = wrap_torch_tensor(torch.from_numpy(idx).cuda()), wrap_torch_tensor(out_t[:, :dim])
    wmb.check(wmb.lib().wholememory_gather(root.wmb_tensor, wi.handle, wo.handle, env, stream, -1))
    torch.cuda.synchronize()
    _assert_convert_kernel(_served_by(), VEC_OF_DIM[dim], True)
    tab = oracle.ShardedTable([table], np.array([0, n_rows], dtype=np.uint64), dim, dim, 0, cv.ORACLE_DT[src])
    oracle.gather(tab, idx, want, dim=dim, out_stride=dim + pad, out_dt=cv.ORACLE_DT[dst])
    nan_in = np.zeros(want.shape, dtype=bool)
    nan_in[valid, :dim] = nan_tab[idx[valid]]
    _compare(cv.from_torch(out_t, dst), want, nan_in, dst, "gather %s -> %s" % (src, dst))
    wgth.destroy_wholememory_tensor(root)

    # ---- scatter: plain rows of the source dtype -> zeroed table of the target dtype, unique ids
    root = wgth.create_wholememory_tensor(comm, mt, "cuda", [n_rows, dim], cv.torch_dtype(dst), [dim, 1])
    local, _ = root.get_local_tensor(host_view=False)
    local.zero_()
    idx = _ids(rng, n_rows, idt)
    valid = idx >= 0
    ws, wi = wrap_torch_tensor(cv.to_torch(table, src).cuda()), wrap_torch_tensor(torch.from_numpy(idx).cuda())
    wmb.check(wmb.lib().wholememory_scatter(ws.handle, wi.handle, root.wmb_tensor, env, stream, -1))
    torch.cuda.synchronize()
    _assert_convert_kernel(_served_by(), VEC_OF_DIM[dim], False)
    want = np.zeros((n_rows, dim), dtype=cv.CARRIER[dst])
    ref = oracle.ShardedTable([want], np.array([0, n_rows], dtype=np.uint64), dim, dim, 0, cv.ORACLE_DT[dst])
    oracle.scatter(table, idx, ref, dim=dim, in_stride=dim, in_dt=cv.ORACLE_DT[src])
    nan_in = np.zeros(want.shape, dtype=bool)
    nan_in[idx[valid]] = nan_tab[valid]
    _compare(cv.from_torch(local, dst), ref.shards[0], nan_in, dst, "scatter %s -> %s" % (src, dst))
    wgth.destroy_wholememory_tensor(root)


@pytest.mark.parametrize("mt", ["continuous", "chunked", "distributed"])
@pytest.mark.parametrize("idt", ["i32", "i64"])
@pytest.mark.parametrize("dim", [64, 66, 65])
@pytest.mark.parametrize("src,dst", cv.FLOAT_PAIRS, ids=lambda v: v)
def test_float_casts_on_boundary_values(gpu_env, src, dst, dim, idt, mt):
    run_pair(gpu_env, src, dst, dim, idt, mt, cv.float_source(src), cv.NAN_COUNT[src])


@pytest.mark.parametrize("idt", ["i32", "i64"])
@pytest.mark.parametrize("dim", [64, 66, 65])
@pytest.mark.parametrize("src,dst", cv.INT_PAIRS, ids=lambda v: v)
def test_int_casts_on_limits(gpu_env, src, dst, dim, idt):
    run_pair(gpu_env, src, dst, dim, idt, "continuous", cv.int_source(src, dst), 0)
