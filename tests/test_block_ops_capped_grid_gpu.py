"""Every block op under a capped grid (WM_AGG_MAX_BLOCKS = 1 and 3), forward and backward, against the references of the
op's own test file.

About fifty launches size their grid through blocks_for() (csrc/kernels/agg_common.cuh), which caps it at 2^20 workgroups;
the kernels stride over their work by the grid. No other test has more work than the cap allows, so the later trips of
those loops — the stride, the ragged last trip, the LDS tile of gat_edge_score_kernel used again, lane groups that share a
wave with one that has left the loop, the inactive lanes of a second column pass on a second target — run here only. The
knob lowers the cap to one and to three workgroups; the block of tests/_capped_block.py then gives every launch a second, a
late and a ragged trip at every lane width (tests/test_capped_block.py asserts that on the CPU).

Per case: one call with the knob unset, one under each cap. Every output of every call is compared with the independent
reference the op's own test uses, imported from there and computed once per case: the numpy restatement of the stated
order, bit for bit; attention alpha within the bound of its float64 softmax, everything downstream restated from the op's
own alpha. The capped calls must also give the bits of the uncapped one. wholememory_ext_agg_grid_stats tells how many
launches blocks_for() sized and how many of them the cap cut short: none with the knob unset, some under cap 3, and under
cap 1 all but the number written beside the case (`full`), whose comment names the launch sites that fit one workgroup
at that shape.

A row that a capped kernel fails to write must not pass for written: the ops allocate their outputs uninitialised, and the
allocator would hand a capped call the very memory that held the right answer of the call before it. So the device
tensors of every call of a case stay alive until the case ends. The scratch of a backward (partial rows, da / dz / ds, the
logits) is freed after every call and would likewise come back to the next call with the right contents in it: a chunk
kernel that skipped a tile could read the partial row its predecessor wrote. So every checked call follows a call of the same
op on other data of the same shapes (the rows of every input reversed), whose scratch has the same sizes and lands in the
same places: what a kernel fails to write is then stale from other data by construction. On top of that the free blocks
of the allocator, small and large, are filled with NaN patterns before each checked call (poison()).

Row widths of the agg_concat family (fp32 rows; lanes_for and use_vec4 decide): 8 (two 16-byte pieces, 16 lanes), 128 (32
pieces, 32 lanes), 320 (80 pieces, 64 lanes, a second column pass with 48 inactive lanes), 3 (element-wise, 16 lanes) and 33
(element-wise, 64 lanes). 16-bit rows have 8 elements to a piece: 8 (16 lanes), 256 (32 pieces, 32 lanes), 640 (80 pieces,
64 lanes and the second pass), 3 and 33. The quantized table goes by dwords of 4 codes: 8, 128 and 320 as above, 3 and 33
(ragged last dword, 16 lanes) and 131 (33 dwords: the 64-lane kernel with the ragged store).

(H, F) of the attention ops. mha_gat_n2n and the edge-feature op take 16-byte pieces whenever F % 4 == 0:
  (2, 4) 2 pieces, 16 lanes; (2, 64) 32 pieces, 32 lanes; (2, 160) 80 pieces, 64 lanes and the second column pass;
  element-wise (2, 3) 6 columns, 16 lanes; (2, 9) 18 columns, 32 lanes (test_gat_gpu reaches it with H = 8, F = 3);
  (3, 11) 33 columns, 64 lanes.
mha_gat_v2_n2n and mha_simple_n2n split the tree of a head over lanes only when F is a power of two:
  (2, 4) 16 lanes; (2, 64) 32 lanes; (3, 128) 96 pieces, 64 lanes, a second column pass with 32 inactive lanes — the forward
  and the per-target backward; (2, 160) runs those two element-wise (320 columns, 64 lanes, five passes, with the dot
  kernels in front) and the per-source walk on 16-byte pieces at 64 lanes; (2, 3), (2, 9), (3, 11) element-wise at 16, 32
  and 64 lanes.
The per-source walk (the chunk and fold kernels) goes by its own width, on 16-byte pieces whenever F % 4 == 0. For
mha_gat_n2n, the edge-feature op and mha_gat_v2_n2n it is H F columns wide, the lane widths as listed above ((3, 128) and
(2, 160): 64 lanes on 16-byte pieces). For mha_simple_n2n it is 2 H F columns wide (grad_key, then grad_value):
  16-byte pieces: (2, 4) 16 columns, 4 pieces, 16 lanes; (2, 32) 128 columns, 32 pieces, 32 lanes; (2, 64) 64 pieces,
  (3, 128) 192 pieces and (2, 160) 160 pieces, 64 lanes;
  element-wise: (2, 3) 12 columns, 16 lanes; (2, 5) 20 columns, 32 lanes (test_tconv_gpu reaches it with the same shape);
  (2, 9) 36 columns and (3, 11) 66 columns, 64 lanes.
Its forward and per-target backward at (2, 32) and (2, 5): 16 pieces and 10 columns, 16 lanes."""
import ctypes as C

import numpy as np
import pytest

import _capped_block as CB

pytestmark = pytest.mark.gpu

F32 = np.float32
KNOB = "WM_AGG_MAX_BLOCKS"
CAPS = (1, 3)
WIDTHS = [8, 128, 320, 3, 33]
WIDTHS16 = [8, 256, 640, 3, 33]
WIDTHS_Q = [8, 128, 320, 3, 33, 131]
AGGRS = ["mean", "sum"]
_ALIVE = []   # the device tensors behind the outputs of the running case: kept, so that no later call reuses their memory


# ---------------------------------------------------------------- the harness
def from_alpha(refs, al, make):
    """references restated from the op's own alpha, kept in the case's `refs`: made once per case, again only if a call's
    alpha has other bits"""
    if refs.get("alpha") != al.tobytes():
        refs["alpha"], refs["made"] = al.tobytes(), make()
    return refs["made"]


def alt(a, other):
    """the array, or for the call on other data its rows reversed"""
    return np.ascontiguousarray(a[::-1]) if other else a


def the_block():
    from wholegraph_amd.torch.aggregation import chunk_edges
    C_ = chunk_edges()
    row_ptr, col = CB.capped_block(C_)
    return C_, row_ptr, col


def grid_stats():
    """(launches sized by blocks_for(), those the cap cut short) since the last call"""
    from wholegraph_amd import binding as wmb
    launches, truncated = C.c_int64(-1), C.c_int64(-1)
    wmb.lib().wholememory_ext_agg_grid_stats(C.byref(launches), C.byref(truncated))
    return launches.value, truncated.value


def np_of(t):
    """the bits of a device tensor (16-bit floats as their uint16 patterns); the tensor stays alive until the case ends"""
    import torch
    _ALIVE.append(t)
    t = t.detach().contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    view = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    differ = got.view(view) != want.view(view)
    assert not differ.any(), "%s: %d of %d elements differ from the reference, first at %s" % (
        what, int(differ.sum()), differ.size, tuple(np.argwhere(differ)[0]))


def poison():
    """NaN patterns into free memory of the caching allocator's small and large pools, where the next outputs will land"""
    import torch
    # int32 elements: 16 blocks each of 512 B, 4, 32 and 256 KiB, then 0.8, 3, 9 and 64 MiB
    sizes = [128] * 16 + [1 << 10] * 16 + [8 << 10] * 16 + [64 << 10] * 16 + [200 << 10] * 12 + [768 << 10] * 6 + \
        [2304 << 10] * 4 + [16 << 20]
    junk = [torch.full((n,), -1, dtype=torch.int32, device="cuda") for n in sizes]
    del junk


def sweep(knobs, run, check, full, what, scramble=True):
    """run(other) -> {name: numpy array} is one forward and backward of the op, on the case's inputs or, with `other`, on
    other data of the same shapes; check(outs, label) compares every output with the reference. Checked with the knob unset,
    then under each cap, each time behind an unchecked, uncapped call on the other data (`scramble`: not for the forward-only
    table ops, which have no scratch); `full` = the launches of one call that fit one workgroup."""
    try:
        _sweep(knobs, run, check, full, what, scramble)
    finally:
        _ALIVE.clear()


def _sweep(knobs, run, check, full, what, scramble):
    import torch
    plain, plain_launches = None, None
    for cap in (None,) + CAPS:
        knobs.unset(KNOB)
        if scramble:
            run(True)
        if cap is not None:
            knobs.set(KNOB, cap)
        label = "%s, %s" % (what, "no cap" if cap is None else "cap %d" % cap)
        poison()
        torch.cuda.synchronize()
        grid_stats()
        outs = run(False)
        torch.cuda.synchronize()
        launches, truncated = grid_stats()
        print("%s: %d launches, %d truncated" % (label, launches, truncated))
        check(outs, label)
        assert launches > 0, label
        if cap is None:
            assert truncated == 0, "%s: %d launches were cut short without a cap" % (label, truncated)
            plain, plain_launches = outs, launches
            continue
        assert launches == plain_launches, "%s: %d launches, %d without a cap" % (label, launches, plain_launches)
        if cap == 1:
            assert launches - truncated == full, "%s: %d of %d launches fit one workgroup, not %d" % (
                label, launches - truncated, launches, full)
        else:
            assert truncated > 0, label
        assert sorted(outs) == sorted(plain)
        for name in outs:
            assert outs[name].tobytes() == plain[name].tobytes(), "%s: %s has other bits than without a cap" % (label, name)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared block is read-only)


# ---------------------------------------------------------------- agg_concat, fp32
# launch sites: agg_forward_kernel (301 targets); agg_bwd_prep_kernel (one thread per edge), agg_bwd_chunk_kernel (21 tiles:
# 2 workgroups of 16 groups), agg_bwd_fold_kernel (1103 sources). Each wants more than one workgroup at every width: full = 0.
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat(gpu_env, knobs, dim, aggr):
    import test_sage_agg_gpu as T
    from wholegraph_amd.torch.aggregation import agg_concat
    C_, row_ptr, col = the_block()

    def make():
        rng = np.random.default_rng(1000 + dim)
        x = rng.standard_normal((CB.N_SRC, dim)).astype(F32)
        g = rng.standard_normal((CB.N_DST, 2 * dim)).astype(F32)
        return x, g, T.ref_forward(row_ptr, col, x, aggr), T.ref_backward(row_ptr, col, g, CB.N_SRC, aggr, C_)

    x_np, g_np, want_out, want_gx = make()

    def run(other):
        x = dev(alt(x_np, other)).requires_grad_(True)
        out = agg_concat(x, dev(row_ptr), dev(col), aggr)
        out.backward(dev(alt(g_np, other)))
        return {"out": np_of(out), "grad_x": np_of(x.grad)}

    def check(o, label):
        same(o["out"], want_out, label + ": out")
        same(o["grad_x"], want_gx, label + ": grad_x")

    sweep(knobs, run, check, 0, "agg_concat %s dim %d" % (aggr, dim))


# ---------------------------------------------------------------- agg_concat, fp16 / bf16
# launch sites: agg16_forward_kernel, agg_bwd_prep_kernel, agg16_bwd_chunk_kernel, agg16_bwd_fold_kernel, as above: full = 0.
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS16)
@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_agg_concat_16_bit(gpu_env, knobs, name, dim, aggr):
    import test_sage_agg_half_gpu as T
    from wholegraph_amd.torch.aggregation import agg_concat
    C_, row_ptr, col = the_block()

    def make():
        rng = np.random.default_rng(2000 + dim)
        xb, x32 = T.random_rows(rng, (CB.N_SRC, dim), name)
        gb, g32 = T.random_rows(rng, (CB.N_DST, 2 * dim), name)
        return (xb, gb, T.round_bits(T.ref_forward(row_ptr, col, x32, aggr), name),
                T.round_bits(T.ref_backward(row_ptr, col, g32, CB.N_SRC, aggr, C_), name))

    xb, gb, want_out, want_gx = make()

    def run(other):
        x = T.dev16(alt(xb, other), name).requires_grad_(True)
        out = agg_concat(x, dev(row_ptr), dev(col), aggr)
        out.backward(T.dev16(alt(gb, other), name))
        assert out.dtype == T.tdtype(name) and x.grad.dtype == T.tdtype(name)
        return {"out": np_of(out), "grad_x": np_of(x.grad)}

    def check(o, label):
        same(o["out"], want_out, label + ": out")
        same(o["grad_x"], want_gx, label + ": grad_x")

    sweep(knobs, run, check, 0, "agg_concat %s %s dim %d" % (name, aggr, dim))


# ---------------------------------------------------------------- agg_concat_weighted
# launch sites: aggw_forward_kernel, agg_bwd_prep_kernel, aggw_bwd_chunk_kernel, aggw_bwd_fold_kernel, and aggw_bwd_weight_kernel
# (a group per 8 edges: more than 1300 groups). full = 0.
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat_weighted(gpu_env, knobs, dim, aggr):
    import test_weighted_agg_gpu as T
    C_, row_ptr, col = the_block()

    def make():
        rng = np.random.default_rng(3000 + dim)
        x = rng.standard_normal((CB.N_SRC, dim)).astype(F32)
        w = rng.standard_normal(len(col)).astype(F32)
        g = rng.standard_normal((CB.N_DST, 2 * dim)).astype(F32)
        return (x, w, g) + tuple(T.ref_all(row_ptr, col, w, x, g, aggr, C_))

    x_np, w_np, g_np, want_out, want_gx, want_gw = make()

    def run(other):
        out, gx, gw = T.run_op(alt(x_np, other), np.array(row_ptr), np.array(col), alt(w_np, other), alt(g_np, other), aggr)
        return {"out": np_of(out), "grad_x": np_of(gx), "grad_w": np_of(gw)}

    def check(o, label):
        same(o["out"], want_out, label + ": out")
        same(o["grad_x"], want_gx, label + ": grad_x")
        same(o["grad_w"], want_gw, label + ": grad_w")

    # (the op keeps a bounded record of its last backward calls for test_weighted_agg_gpu.py, which counts on room in it:
    # left as it was found)
    import wholegraph_amd.torch.weighted_aggregation as wa
    record = list(wa.backward_requests)
    try:
        sweep(knobs, run, check, 0, "agg_concat_weighted %s dim %d" % (aggr, dim))
    finally:
        wa.backward_requests[:] = record


# ---------------------------------------------------------------- agg_concat_rel
# launch sites: relagg_fwd_kernel (targets of at most LANES edges take the one-round path, the others a round per relation:
# degree 17 and 65 are beyond 16 and 64 lanes), agg_bwd_prep_kernel, relagg_chunk_bwd_kernel, relagg_fold_bwd_kernel. full = 0.
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat_rel(gpu_env, knobs, dim, aggr):
    import test_rel_agg_gpu as T
    C_, row_ptr, col = the_block()
    R = 3

    def make():
        rng = np.random.default_rng(4000 + dim)
        et = rng.integers(0, R, len(col)).astype(np.int32)
        et[rng.random(len(col)) < 0.02] = R            # types out of range: they keep their place and add nothing
        et[rng.random(len(col)) < 0.02] = -1
        x = rng.standard_normal((CB.N_SRC, dim)).astype(F32)
        g = rng.standard_normal((CB.N_DST, (R + 1) * dim)).astype(F32)
        want_out, want_scale = T.ref_forward(row_ptr, col, et, R, x, aggr)
        return x, et, g, want_out, want_scale, T.ref_grad_x(row_ptr, col, et, R, want_scale, g, CB.N_SRC, C_, aggr)

    x_np, et, g_np, want_out, want_scale, want_gx = make()

    def run(other):
        out, scale, gx = T.run_op(alt(x_np, other), np.array(row_ptr), np.array(col), et, R, alt(g_np, other), aggr)
        o = {"out": np_of(out), "grad_x": np_of(gx)}
        assert (scale is not None) == (aggr == "mean")
        if scale is not None:
            o["edge_scale"] = np_of(scale)
        return o

    def check(o, label):
        same(o["out"], want_out, label + ": out")
        if aggr == "mean":
            same(o["edge_scale"], want_scale, label + ": edge_scale")
        same(o["grad_x"], want_gx, label + ": grad_x")

    sweep(knobs, run, check, 0, "agg_concat_rel %s dim %d" % (aggr, dim))


# ---------------------------------------------------------------- gather_agg_concat from a chunked table (forward only)
# launch site: aggg_forward_kernel. full = 0.
@pytest.mark.parametrize("dtype,dim", [("float32", d) for d in WIDTHS] + [("bfloat16", 256), ("float16", 33)])
def test_gather_agg_concat(gpu_env, knobs, dtype, dim):
    import torch
    import test_gather_agg_gpu as T
    import wholegraph_amd.torch as wgth
    from wholegraph_amd.torch import gather_aggregation
    C_, row_ptr, col = the_block()
    n_rows = 5003

    def make():
        rng = np.random.default_rng(5000 + dim)
        values = T.table_values(rng, n_rows, dim, getattr(torch, dtype))
        ids = rng.integers(0, n_rows, CB.N_SRC)
        ids[:3] = [0, n_rows - 1, 0]
        x = values.float().numpy()[ids]
        return values, ids, {aggr: T.ref_forward(row_ptr, col, x, aggr) for aggr in AGGRS}

    values, ids_np, want = make()
    emb = T.make_embedding(gpu_env, "chunked", "cuda", getattr(torch, dtype), values)
    try:
        for aggr in AGGRS:
            def run(other):
                before = gather_aggregation.calls()
                out = wgth.gather_agg_concat(emb, dev(ids_np), dev(row_ptr), dev(col), aggr)
                assert gather_aggregation.calls() == before + 1, "the fused kernel did not run"
                return {"out": np_of(out)}

            sweep(knobs, run, lambda o, label: same(o["out"], want[aggr], label + ": out"), 0,
                  "gather_agg_concat %s %s dim %d" % (dtype, aggr, dim), scramble=False)
    finally:
        wgth.destroy_embedding(emb)


# ---------------------------------------------------------------- gather_agg_concat from an 8-bit quantized table (forward only)
# launch site: aggq_forward_kernel. full = 0.
@pytest.mark.parametrize("dim", WIDTHS_Q)
def test_gather_agg_concat_quantized(gpu_env, knobs, dim):
    import test_qagg_gpu as T
    import wholegraph_amd.torch as wgth
    from test_qrows_gpu import destroy, make_table, raw_of, reference
    from wholegraph_amd.torch import gather_aggregation
    C_, row_ptr, col = the_block()
    n_rows = T.N_ROWS
    x, _, _ = reference(n_rows, dim)
    t = make_table(gpu_env, "chunked", "cuda", x, row_align=4)
    try:
        def make():
            ids = np.random.default_rng(6000 + dim).integers(0, n_rows, CB.N_SRC)
            ids[:3] = [0, n_rows - 1, 0]
            raw = raw_of(t).cpu().numpy().view(np.uint8)   # the table's bytes, read by the row gather (no block op)
            return ids, {aggr: T.numpy_forward(raw, dim, ids, row_ptr, col, aggr) for aggr in AGGRS}

        knobs.unset(KNOB)
        ids_np, want = make()
        for aggr in AGGRS:
            def run(other):
                before = gather_aggregation.quantized_calls()
                out = wgth.gather_agg_concat(t, dev(ids_np), dev(row_ptr), dev(col), aggr)
                assert gather_aggregation.quantized_calls() == before + 1, "the fused kernel did not run"
                return {"out": np_of(out)}

            sweep(knobs, run, lambda o, label: same(o["out"], want[aggr], label + ": out"), 0,
                  "quantized gather_agg_concat %s dim %d" % (aggr, dim), scramble=False)
    finally:
        destroy(t)


# ---------------------------------------------------------------- agg_concat_pna, all five aggregators
# launch sites: pna_fwd_kernel, agg_bwd_prep_kernel, pna_bwd_chunk_kernel, pna_bwd_fold_kernel. full = 0.
@pytest.mark.parametrize("dim", WIDTHS)
def test_agg_concat_pna(gpu_env, knobs, dim):
    import test_pna_gpu as T
    C_, row_ptr, col = the_block()
    names = T.ORDER

    def make():
        rng = np.random.default_rng(7000 + dim)
        x = rng.standard_normal((CB.N_SRC, dim)).astype(F32)
        x[:, 0] = 2.0                                   # ties in min / max, a variance of exactly zero
        g = rng.standard_normal((CB.N_DST, (len(names) + 1) * dim)).astype(F32)
        want_out, saved = T.ref_forward(row_ptr, col, x, names)
        return x, g, want_out, saved, T.ref_backward(row_ptr, col, x, names, saved, g, C_)

    x_np, g_np, want_out, want_saved, want_gx = make()
    saved_names = ("arg_min", "arg_max", "std_mean", "std_coef")

    def run(other):
        out, saved, gx = T.run_op(alt(x_np, other), np.array(row_ptr), np.array(col), names, alt(g_np, other))
        o = {"out": np_of(out), "grad_x": np_of(gx)}
        assert len(saved) == 4 and all(s is not None for s in saved)
        o.update({n: np_of(s) for n, s in zip(saved_names, saved)})
        return o

    def check(o, label):
        same(o["out"], want_out, label + ": out")
        for n, w in zip(saved_names, want_saved):
            same(o[n], w, label + ": " + n)
        same(o["grad_x"], want_gx, label + ": grad_x")

    sweep(knobs, run, check, 0, "agg_concat_pna dim %d" % dim)


# ---------------------------------------------------------------- the attention ops
def check_alpha(al, ref, bound, label):
    print("%s: alpha max |err| / bound = %.3g" % (label, float(np.max(np.abs(al - ref) / bound))))
    assert (np.abs(al - ref) <= bound).all(), "%s: alpha off by %g" % (label, float(np.max(np.abs(al - ref) / (ref + 1e-30))))


# mha_gat_n2n. Launch sites: gat_score_kernel, gat_fwd_kernel, gat_head_mean_kernel (without concat: 301 F threads);
# gat_bwd_edge_kernel (301 H threads), gat_bwd_prep_kernel, gat_bwd_chunk_kernel, gat_bwd_fold_kernel — more than one workgroup
# at every shape here — and the two sums of grad_att: gat_att_chunk_kernel, a thread per (node chunk, column) = 2 * 2 H F
# threads, and gat_att_fold_kernel, a thread per column = 2 H F threads. Those two fit one workgroup while 4 H F <= 256
# respectively 2 H F <= 256; at (2, 64) the chunk kernel is cut short (512 threads), at (2, 160) both are: every site is cut
# short in at least one case.
GAT_CASES = [
    # H, F, full
    (2, 4, 2),      # gat_att_chunk_kernel (32 threads) and gat_att_fold_kernel (16)
    (2, 64, 1),     # gat_att_fold_kernel (256 threads: exactly one workgroup)
    (2, 160, 0),
    (2, 3, 2),      # gat_att_chunk_kernel (24) and gat_att_fold_kernel (12)
    (2, 9, 2),      # gat_att_chunk_kernel (72) and gat_att_fold_kernel (36)
    (3, 11, 2),     # gat_att_chunk_kernel (132) and gat_att_fold_kernel (66)
]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F,full", GAT_CASES)
def test_mha_gat_n2n(gpu_env, knobs, H, F, full, concat):
    import test_gat_gpu as T
    from wholegraph_amd.torch.gat_aggregation import mha_gat_n2n, node_chunk
    C_, row_ptr, col = the_block()
    refs = {}

    def make():
        rng = np.random.default_rng(8000 + 10 * H + F + concat)
        h, att = T.inputs(rng, CB.N_SRC, H, F)
        G = rng.standard_normal((CB.N_DST, H * F if concat else F)).astype(F32)
        return (h, att, G) + tuple(T.ref_alpha64(row_ptr, col, h, att, H, 0.2))

    h_np, att_np, G_np, ref, bound = make()

    def run(other):
        h, att = dev(alt(h_np, other)).requires_grad_(True), dev(att_np).requires_grad_(True)
        out, alpha = mha_gat_n2n(h, att, dev(row_ptr), dev(col), H, 0.2, concat, return_alpha=True)
        out.backward(dev(alt(G_np, other)))
        return {"out": np_of(out), "alpha": np_of(alpha), "grad_h": np_of(h.grad), "grad_att": np_of(att.grad)}

    def check(o, label):
        al = o["alpha"]
        check_alpha(al, ref, bound, label)
        want_out, (gh, ga) = from_alpha(refs, al, lambda: (
            T.ref_out(row_ptr, col, h_np, al, H, concat),
            T.ref_backward(row_ptr, col, h_np, att_np, al, G_np, H, 0.2, concat, C_, node_chunk())))
        same(o["out"], want_out, label + ": out")
        same(o["grad_h"], gh, label + ": grad_h")
        same(o["grad_att"], ga, label + ": grad_att")

    sweep(knobs, run, check, full, "mha_gat_n2n H %d F %d concat %d" % (H, F, concat))


# The edge-feature GAT. Launch sites: those of mha_gat_n2n, and gat_edge_score_kernel (a workgroup per 256 (edge, head)
# segments, two barriers per slab of 32 columns inside the block-uniform tile loop; F = 64 and 160 take 2 and 5 slabs per tile),
# gat_edge_fwd_kernel, gat_edge_bwd_dz_kernel — cut short at every shape — gat_edge_grad_chunk_kernel, a thread per (chunk of
# 1024 edges, piece of columns) = 11 * H F / 4 threads on 16-byte pieces and 11 * H F element-wise, and
# gat_edge_att_fold_kernel, a thread per column = H F threads. Every site is cut short in at least one case: the four sums
# over chunks all at (2, 160), where even the narrowest, gat_edge_att_fold_kernel, has 320 threads.
GAT_EDGE_CASES = [
    # H, F, full
    (2, 4, 4),      # gat_att_chunk (32 threads), gat_att_fold (16), gat_edge_grad_chunk (22), gat_edge_att_fold (8)
    (2, 64, 2),     # gat_att_fold (256), gat_edge_att_fold (128); gat_edge_grad_chunk has 352 threads
    (2, 160, 0),
    (2, 3, 4),      # gat_att_chunk (24), gat_att_fold (12), gat_edge_grad_chunk (66), gat_edge_att_fold (6)
    (2, 9, 4),      # gat_att_chunk (72), gat_att_fold (36), gat_edge_grad_chunk (198), gat_edge_att_fold (18)
    (3, 11, 3),     # gat_att_chunk (132), gat_att_fold (66), gat_edge_att_fold (33); gat_edge_grad_chunk has 363 threads
]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F,full", GAT_EDGE_CASES)
def test_mha_gat_n2n_with_edge_features(gpu_env, knobs, H, F, full, concat):
    import test_gat_edge_gpu as T
    from test_gat_gpu import inputs, ref_out
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    C_, row_ptr, col = the_block()
    assert (len(col) + node_chunk() - 1) // node_chunk() == 11   # the edge chunks the thread counts above go by
    refs = {}

    def make():
        rng = np.random.default_rng(9000 + 10 * H + F + concat)
        h, att = inputs(rng, CB.N_SRC, H, F)
        att3 = np.concatenate([att, (0.5 * rng.standard_normal(H * F) / np.sqrt(F)).astype(F32)])
        ef = rng.standard_normal((len(col), H * F)).astype(F32)
        G = rng.standard_normal((CB.N_DST, H * F if concat else F)).astype(F32)
        s_edge = T.ref_edge_scores(ef, att3, H)
        return (h, att3, ef, G, s_edge) + tuple(T.ref_alpha64_edge(row_ptr, T.ref_z(row_ptr, col, h, att3, s_edge, H), 0.2))

    h_np, att_np, ef_np, G_np, s_edge, ref, bound = make()

    def run(other):
        out, alpha, es, gh, ga, gef = T.run_op(alt(h_np, other), att_np, dev(alt(ef_np, other)), np.array(row_ptr),
                                               np.array(col), H, concat, alt(G_np, other))
        return {"out": np_of(out), "alpha": np_of(alpha), "edge_scores": np_of(es), "grad_h": np_of(gh),
                "grad_att": np_of(ga), "grad_edge_feat": np_of(gef)}

    def check(o, label):
        same(o["edge_scores"], s_edge, label + ": edge_scores")
        al = o["alpha"]
        check_alpha(al, ref, bound, label)
        want_out, (gh, ga, gef, _) = from_alpha(refs, al, lambda: (
            ref_out(row_ptr, col, h_np, al, H, concat),
            T.ref_backward_edge(row_ptr, col, h_np, att_np, ef_np, al, G_np, H, 0.2, concat, C_, node_chunk())))
        same(o["out"], want_out, label + ": out")
        same(o["grad_h"], gh, label + ": grad_h")
        same(o["grad_att"], ga, label + ": grad_att")
        same(o["grad_edge_feat"], gef, label + ": grad_edge_feat")

    sweep(knobs, run, check, full, "edge GAT H %d F %d concat %d" % (H, F, concat))


# mha_gat_v2_n2n. Launch sites: gatv2_dot_kernel<0> (element-wise only: 301 H threads), gatv2_fwd_kernel, gat_head_mean_kernel;
# gatv2_dot_kernel<1> (element-wise only), gatv2_bwd_dst_kernel, gatv2_bwd_prep_kernel, gatv2_bwd_chunk_kernel,
# gatv2_bwd_fold_kernel — cut short at every shape — and the sums of grad_att over the 301 targets' one node chunk:
# gatv2_att_chunk_kernel and gatv2_att_fold_kernel, a thread per column = H F threads each: cut short at (3, 128) and (2, 160).
GATV2_CASES = [
    # H, F, full
    (2, 4, 2),      # gatv2_att_chunk_kernel and gatv2_att_fold_kernel (8 threads each)
    (2, 64, 2),     # (128 threads each)
    (3, 128, 0),    # 384 columns
    (2, 160, 0),    # 320 columns
    (2, 3, 2),      # (6 each)
    (2, 9, 2),      # (18 each)
    (3, 11, 2),     # (33 each)
]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F,full", GATV2_CASES)
def test_mha_gat_v2_n2n(gpu_env, knobs, H, F, full, concat):
    import test_gatv2_gpu as T
    from test_gat_gpu import ref_out
    from wholegraph_amd.torch.gat_aggregation import node_chunk
    C_, row_ptr, col = the_block()
    slope = 0.2
    refs = {}

    def make():
        rng = np.random.default_rng(10000 + 10 * H + F + concat)
        hs, hd, att = T.inputs(rng, CB.N_SRC, CB.N_DST, H, F)
        G = rng.standard_normal((CB.N_DST, H * F if concat else F)).astype(F32)
        l32, _, _ = T.ref_logits(row_ptr, col, hs, hd, att, H, slope)
        return (hs, hd, att, G) + tuple(T.ref_alpha64(row_ptr, l32))

    hs_np, hd_np, att_np, G_np, ref, bound = make()

    def run(other):
        out, alpha, grads = T.run_op(dev(alt(hs_np, other)), dev(alt(hd_np, other)), att_np, np.array(row_ptr), np.array(col),
                                     alt(G_np, other), H, slope, concat)
        return {"out": np_of(out), "alpha": np_of(alpha), "grad_h_src": np_of(grads[0]), "grad_h_dst": np_of(grads[1]),
                "grad_att": np_of(grads[2])}

    def check(o, label):
        al = o["alpha"]
        check_alpha(al, ref, bound, label)
        want_out, (ghs, ghd, ga) = from_alpha(refs, al, lambda: (
            ref_out(row_ptr, col, hs_np, al, H, concat),
            T.ref_backward(row_ptr, col, hs_np, hd_np, att_np, al, G_np, H, slope, concat, C_, node_chunk())))
        same(o["out"], want_out, label + ": out")
        same(o["grad_h_src"], ghs, label + ": grad_h_src")
        same(o["grad_h_dst"], ghd, label + ": grad_h_dst")
        same(o["grad_att"], ga, label + ": grad_att")

    sweep(knobs, run, check, full, "mha_gat_v2_n2n H %d F %d concat %d" % (H, F, concat))


# mha_simple_n2n. Launch sites: tconv_dot_kernel<0> (element-wise only), tconv_fwd_kernel, gat_head_mean_kernel;
# tconv_dot_kernel<1> (element-wise only), tconv_bwd_dst_kernel, tconv_bwd_prep_kernel, tconv_bwd_chunk_kernel,
# tconv_bwd_fold_kernel. There is no column sum: every launch is cut short at every shape, full = 0.
# The walk is 2 H F columns wide: (2, 5), 20 columns, is its element-wise instantiation at 32 lanes (the docstring above
# lists the lane width of every shape).
TCONV_SHAPES = [(2, 4), (2, 32), (2, 64), (3, 128), (2, 160), (2, 3), (2, 5), (2, 9), (3, 11)]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,F", TCONV_SHAPES)
def test_mha_simple_n2n(gpu_env, knobs, H, F, concat):
    import test_tconv_gpu as T
    from test_gat_gpu import ref_out
    from test_gatv2_gpu import ref_alpha64
    C_, row_ptr, col = the_block()
    norm = True
    refs = {}

    def make():
        rng = np.random.default_rng(11000 + 10 * H + F + concat)
        k, q, v = T.inputs(rng, CB.N_SRC, CB.N_DST, H, F)
        G = rng.standard_normal((CB.N_DST, H * F if concat else F)).astype(F32)
        return (k, q, v, G) + tuple(ref_alpha64(row_ptr, T.ref_logits(row_ptr, col, k, q, H, norm)))

    k_np, q_np, v_np, G_np, ref, bound = make()

    def run(other):
        out, alpha, grads = T.run_op(dev(alt(k_np, other)), dev(alt(q_np, other)), dev(alt(v_np, other)), np.array(row_ptr),
                                     np.array(col), alt(G_np, other), H, concat, norm)
        return {"out": np_of(out), "alpha": np_of(alpha), "grad_key": np_of(grads[0]), "grad_query": np_of(grads[1]),
                "grad_value": np_of(grads[2])}

    def check(o, label):
        al = o["alpha"]
        check_alpha(al, ref, bound, label)
        want_out, (gk, gq, gv) = from_alpha(refs, al, lambda: (
            ref_out(row_ptr, col, v_np, al, H, concat),
            T.ref_backward(row_ptr, col, k_np, q_np, v_np, al, G_np, H, concat, norm, C_)))
        same(o["out"], want_out, label + ": out")
        same(o["grad_key"], gk, label + ": grad_key")
        same(o["grad_query"], gq, label + ": grad_query")
        same(o["grad_value"], gv, label + ": grad_value")

    sweep(knobs, run, check, 0, "mha_simple_n2n H %d F %d concat %d" % (H, F, concat))


# ---------------------------------------------------------------- the knob itself
def test_values_that_are_no_positive_integer_leave_the_cap_alone(gpu_env, knobs):
    """empty, zero, negative, not a number, trailing text: the default cap, nothing cut short; a value beyond 2^20 is 2^20"""
    import test_sage_agg_gpu as T
    from wholegraph_amd.torch.aggregation import agg_concat
    C_, row_ptr, col = the_block()
    x_np = np.random.default_rng(12000).standard_normal((CB.N_SRC, 8)).astype(F32)
    want_out = T.ref_forward(row_ptr, col, x_np, "mean")
    for value in ("", "0", "-3", "many", "3 blocks", str(1 << 40)):
        knobs.set(KNOB, value)
        poison()
        grid_stats()
        out = agg_concat(dev(x_np), dev(row_ptr), dev(col), "mean")
        launches, truncated = grid_stats()
        assert (launches, truncated) == (1, 0), (value, launches, truncated)
        same(np_of(out), want_out, "WM_AGG_MAX_BLOCKS=%r" % value)
    knobs.set(KNOB, "2")
    poison()
    grid_stats()
    out = agg_concat(dev(x_np), dev(row_ptr), dev(col), "mean")
    assert grid_stats() == (1, 1)
    same(np_of(out), want_out, "WM_AGG_MAX_BLOCKS=2")
    _ALIVE.clear()
