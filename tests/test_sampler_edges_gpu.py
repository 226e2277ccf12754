"""The neighbour samplers on a degree ladder and on degenerate edge weights (MI355X).

The sampler kernels of csrc/kernels/graph.hip only do real work on a centre whose degree exceeds max_sample_count (M), and
they branch on M and on the degree: two register kernels (M <= 32, two centres per wave; M <= 64), the LDS kernel up to
M = 1024, the reservoir above it (32 virtual threads, a new round every 32 candidates); for the weighted sampler the two
register kernels and the LDS candidate list (128 or 256 virtual threads, capacity P = power of two >= 2M, compacted whenever
it holds more than P - 64 keys, above 64 KiB on the raised dynamic-LDS limit). The ladder graph has one node per degree around
every one of these branch points, so that for every fan-out run here several centres draw and degrees M - 1, M, M + 1 (and
M + 31 ... M + 33 for the reservoir) are present; the number of centres is odd, so the last wave of the two-centres-per-wave
kernels has a dead second group.

The weight classes add what no other test has: zero weights (key -inf, whole groups of keys tie and the neighbour index
decides), weights whose reciprocal overflows or is subnormal in float32, +inf (key -0) and float64 weights outside float32's
range. NaN and negative weights are outside the sampler's contract.

Every comparison with the CPU oracle is exact and ordered; the oracle's outputs are computed once per (weights, fan-out) and
shared by the cases. tests/test_graph_oracle.py pins the oracle itself on these inputs without a GPU."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the ladder graph
LADDER_DEGREES = tuple(sorted(set(range(0, 321)) | {
    383, 384, 385, 511, 512, 513, 639, 640, 641,
    1023, 1024, 1025, 1026, 1027, 1056, 1057, 1087, 1088, 1089,
    2047, 2048, 2049, 2050, 2051, 3000,
    4095, 4096, 4097, 4098, 8191, 8192, 8193, 16383, 16384, 16385}))

UNWEIGHTED_FANOUTS = (-1, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1026, 2048, 2049,
                      4096, 4097, 16384)
UNWEIGHTED_SUBSET = (1, 33, 65, 1024, 1025)          # the DISTRIBUTED CSR (positions-only kernels)
WEIGHTED_FANOUTS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 4095, 4096, 8191, 8192)
WEIGHTED_SUBSET = (1, 33, 65, 257, 1024)
WEIGHT_CLASSES = ("ordinary", "zeros", "half_zero", "equal", "extremes32", "extremes64")

_LADDERS = {}
_WEIGHTS = {}
_REFERENCE = {}


def ladder_graph(max_degree=None):
    """-> row_ptr int64, col int64, centres int64 (read-only, shared). One node per degree of LADDER_DEGREES (up to max_degree),
    node order shuffled, columns random node ids; the centres are every node once in a second shuffled order plus three
    repeats of earlier nodes — an odd number."""
    if max_degree not in _LADDERS:
        rng = np.random.default_rng(20261019)
        deg = np.array([d for d in LADDER_DEGREES if max_degree is None or d <= max_degree], dtype=np.int64)
        rng.shuffle(deg)
        n_nodes = deg.shape[0]
        row_ptr = np.zeros(n_nodes + 1, dtype=np.int64)
        np.cumsum(deg, out=row_ptr[1:])
        col = rng.integers(0, n_nodes, int(row_ptr[-1])).astype(np.int64)
        centers = rng.permutation(n_nodes).astype(np.int64)
        centers = np.concatenate([centers, centers[[5, n_nodes // 2, 0]]])
        if centers.shape[0] % 2 == 0:
            centers = np.concatenate([centers, centers[[7]]])
        for a in (row_ptr, col, centers):
            a.setflags(write=False)
        _LADDERS[max_degree] = (row_ptr, col, centers)
    return _LADDERS[max_degree]


def center_degrees(row_ptr, centers):
    c = centers.astype(np.int64)
    return row_ptr[c + 1] - row_ptr[c]


def assert_ladder_classes(row_ptr, centers, m, max_degree=None):
    """the centres hold what the ladder promises for this fan-out: an odd number of them, at least 8 that draw (or as many
    as the ladder has degrees above m), and degrees m - 1, m, m + 1 where the ladder has them — a later change of the
    generator cannot silently empty a class"""
    assert centers.shape[0] % 2 == 1, "the number of centres must be odd (a dead second group in the last wave)"
    deg = center_degrees(row_ptr, centers)
    ladder = [d for d in LADDER_DEGREES if max_degree is None or d <= max_degree]
    if m <= 0:
        return deg
    above = sum(1 for d in ladder if d > m)
    assert int((deg > m).sum()) >= min(8, above), "only %d centres draw at max_sample_count %d" % (int((deg > m).sum()), m)
    for d in (m - 1, m, m + 1):
        if d in ladder:
            assert (deg == d).any(), "no centre of degree %d for max_sample_count %d" % (d, m)
    return deg


def ladder_weights(cls, n_edges):
    """one weight per edge for the named class, fixed seed (read-only, shared)"""
    key = (cls, n_edges)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    rng = np.random.default_rng(7919 + WEIGHT_CLASSES.index(cls))
    f32 = np.finfo(np.float32)
    if cls == "ordinary":          # 10^U(-6, 6) with runs of equal values: every 7th edge, and 700 edges in a row every 5000
        w = np.power(10.0, rng.uniform(-6.0, 6.0, n_edges))
        w[::7] = 1.0
        for start in range(0, n_edges, 5000):
            w[start:start + 700] = 0.25
        w = w.astype(np.float32)
    elif cls == "zeros":
        w = np.zeros(n_edges, dtype=np.float32)
    elif cls == "half_zero":
        w = np.where(rng.random(n_edges) < 0.5, 0.0, rng.random(n_edges)).astype(np.float32)
    elif cls == "equal":
        w = np.ones(n_edges, dtype=np.float64)
    elif cls == "extremes32":
        with np.errstate(all="ignore"):
            values = np.array([0.0, 1e-45, 1e-39, 2.9e-39, 3e-39, f32.tiny, 1e-30, 0.5, 1.0, 1.0, 1.0, 2.0, 1e30, 3e38, np.inf],
                              dtype=np.float64).astype(np.float32)
        assert values[1] > 0 and values[2] < f32.tiny and np.isinf(values[-1])     # subnormals survive the cast here
        w = values[rng.integers(0, values.shape[0], n_edges)]
    elif cls == "extremes64":
        values = np.array([0.0, 5e-324, 1e-320, 1e-60, 1e-46, 7e-46, 1e-39, 1e-38, 1.0, 1.0, 1.0, 3.4028235e38, 3.4028236e38,
                           1e39, 1e300, np.inf], dtype=np.float64)
        w = values[rng.integers(0, values.shape[0], n_edges)]
    else:
        raise KeyError(cls)
    w.setflags(write=False)
    _WEIGHTS[key] = w
    return w


def as_float32(weights):
    """what the kernel's static_cast<float> gives (IEEE round to nearest: overflow to inf, underflow to subnormal or 0)"""
    with np.errstate(all="ignore"):
        return weights.astype(np.float32)


def weighted_seed(m):
    return 1234567 * m + 987654321987


def unweighted_seed(m):
    return 1000003 * (m + 5) + 12345678901234567


def host_statement_keys(weights32, s, n, c, m, seed):
    """the A-Res keys of one centre (position c of the batch, row [s, s + n)) from the streams the reference's host
    statement numbers: virtual thread t of a block of 128 (256 when m > 256) keys neighbours t, t + block, ... consecutively
    from stream c * block + t"""
    block = 256 if m > 256 else 128
    keys = np.empty(n, dtype=np.float32)
    for t in range(min(block, n)):
        sel = np.arange(t, n, block)
        keys[sel] = oracle.weighted_keys(seed, c * block + t, weights32[s + sel])
    return keys


def assert_no_nan_keys(row_ptr, centers, weights, m, seed):
    """CPU only: the oracle's comparator is a total order only without NaN keys (NaN needs -inf * 0, a 2^-25 event per draw on
    a +inf weight). Checked on a sample of the drawing centres: the first, the last, the one of the highest degree."""
    deg = center_degrees(row_ptr, centers)
    drawing = np.nonzero(deg > m)[0]
    if drawing.shape[0] == 0:
        return
    w32 = as_float32(weights)
    for c in sorted({int(drawing[0]), int(drawing[-1]), int(drawing[np.argmax(deg[drawing])])}):
        keys = host_statement_keys(w32, int(row_ptr[centers[c]]), int(deg[c]), c, m, seed)
        assert not np.isnan(keys).any(), "NaN key at centre %d, max_sample_count %d: choose another seed" % (c, m)


def unweighted_reference(m):
    key = ("unweighted", m)
    if key not in _REFERENCE:
        row_ptr, col, centers = ladder_graph()
        _REFERENCE[key] = oracle.sample_unweighted(row_ptr, col, centers, m, unweighted_seed(m))
    return _REFERENCE[key]


def weighted_reference(cls, m):
    key = (cls, m)
    if key not in _REFERENCE:
        row_ptr, col, centers = ladder_graph()
        weights = ladder_weights(cls, col.shape[0])
        assert_no_nan_keys(row_ptr, centers, weights, m, weighted_seed(m))
        _REFERENCE[key] = oracle.sample_weighted(row_ptr, col, weights, centers, m, weighted_seed(m))
    return _REFERENCE[key]


# ------------------------------------------------------------------------------------------------ oracle-independent checks
def assert_sample_structure(row_ptr, centers, m, off, egid):
    """per centre min(degree, M) distinct edge ids, every one inside the centre's row"""
    deg = center_degrees(row_ptr, centers)
    cnt = deg if m <= 0 else np.minimum(deg, m)
    assert np.array_equal(np.diff(off.astype(np.int64)), cnt), "per-centre counts at max_sample_count=%d" % m
    pos = np.repeat(np.arange(centers.shape[0]), cnt)
    c = centers.astype(np.int64)[pos]
    assert np.all((egid >= row_ptr[c]) & (egid < row_ptr[c + 1])), "edge id outside its row at max_sample_count=%d" % m
    pairs = pos.astype(np.int64) * int(row_ptr[-1] + 1) + egid
    assert np.unique(pairs).shape[0] == pairs.shape[0], "an edge sampled twice at max_sample_count=%d" % m


def assert_zero_weight_order(row_ptr, centers, weights, m, off, egid):
    """weights >= 0 with zeros among them. A zero weight gives the key -inf, below every key of a positive weight, and equal
    keys go by neighbour index. So a drawing centre returns min(#positive, M) positive-weight neighbours first, then the
    LOWEST-index zero-weight neighbours in ascending order (all weights zero: its first M neighbours)."""
    deg = center_degrees(row_ptr, centers)
    for c in np.nonzero(deg > m)[0]:
        s = int(row_ptr[centers[c]])
        picks = egid[off[c]:off[c + 1]]
        row_positive = weights[s:s + int(deg[c])] > 0
        n_pos = min(int(row_positive.sum()), m)
        picked_positive = weights[picks] > 0
        assert int(picked_positive.sum()) == n_pos, "centre %d, max_sample_count %d: positive-weight picks" % (c, m)
        assert picked_positive[:n_pos].all(), "centre %d, max_sample_count %d: a zero weight before a positive one" % (c, m)
        zero_ids = s + np.nonzero(~row_positive)[0][:m - n_pos]
        assert np.array_equal(picks[n_pos:], zero_ids), "centre %d, max_sample_count %d: zero-weight picks" % (c, m)


# ------------------------------------------------------------------------------------------------ unweighted
def _wm_array(comm, mt, arr):
    from test_weighted_chain_gpu import _wm_array as wm_array
    return wm_array(comm, mt, np.array(arr))        # (a writable copy: the shared arrays are read-only)


def _destroy(ts):
    from test_weighted_chain_gpu import _destroy as destroy
    destroy(ts)


@pytest.mark.parametrize("mt", ["continuous", "chunked", "distributed"])
@pytest.mark.parametrize("center_dtype,col_dtype", [(np.int64, np.int64), (np.int32, np.int32), (np.int64, np.int32),
                                                    (np.int32, np.int64)])
def test_unweighted_ladder_equals_the_oracle(gpu_env, mt, center_dtype, col_dtype):
    import torch
    import wholegraph_amd.torch as wgth
    row_ptr, col, centers = ladder_graph()
    ts = [_wm_array(gpu_env, mt, row_ptr), _wm_array(gpu_env, mt, col.astype(col_dtype))]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    dev_centers = torch.from_numpy(centers.astype(center_dtype)).cuda()
    for m in (UNWEIGHTED_SUBSET if mt == "distributed" else UNWEIGHTED_FANOUTS):
        assert_ladder_classes(row_ptr, centers, m)
        off, ids, lid, egid = g.unweighted_sample_without_replacement_one_hop(
            dev_centers, m, random_seed=unweighted_seed(m), need_center_local_output=True, need_edge_output=True)
        o_off, o_ids, o_lid, o_egid = unweighted_reference(m)
        assert off.dtype == torch.int32 and lid.dtype == torch.int32 and egid.dtype == torch.int64
        assert ids.dtype == torch.from_numpy(np.empty(0, dtype=col_dtype)).dtype
        off, ids, lid, egid = [t.cpu().numpy() for t in (off, ids, lid, egid)]
        assert np.array_equal(off, o_off), "offsets differ at max_sample_count=%d" % m
        assert_sample_structure(row_ptr, centers, m, off, egid)
        assert np.array_equal(egid, o_egid), "edge ids differ at max_sample_count=%d" % m
        assert np.array_equal(ids, o_ids.astype(col_dtype)), "sampled ids differ at max_sample_count=%d" % m
        assert np.array_equal(lid, o_lid), "centre local ids differ at max_sample_count=%d" % m
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ weighted
def _weighted_structure(comm, mt, col_dtype, weights):
    import wholegraph_amd.torch as wgth
    row_ptr, col, _ = ladder_graph()
    ts = [_wm_array(comm, mt, row_ptr), _wm_array(comm, mt, col.astype(col_dtype)), _wm_array(comm, mt, weights)]
    g = wgth.GraphStructure()
    g.set_csr_graph(ts[0], ts[1])
    g.set_edge_attribute("w", ts[2])
    return g, ts


@pytest.mark.parametrize("cls", WEIGHT_CLASSES)
@pytest.mark.parametrize("mt,center_dtype,col_dtype,fanouts", [
    ("continuous", np.int64, np.int64, WEIGHTED_FANOUTS), ("continuous", np.int32, np.int32, WEIGHTED_FANOUTS),
    ("continuous", np.int64, np.int32, WEIGHTED_SUBSET), ("continuous", np.int32, np.int64, WEIGHTED_SUBSET),
    ("chunked", np.int64, np.int64, WEIGHTED_SUBSET), ("distributed", np.int32, np.int64, WEIGHTED_SUBSET)],
    ids=["continuous-i64-i64-full", "continuous-i32-i32-full", "continuous-i64-i32-subset", "continuous-i32-i64-subset",
         "chunked-i64-i64-subset", "distributed-i32-i64-subset"])
def test_weighted_ladder_equals_the_oracle(gpu_env, cls, mt, center_dtype, col_dtype, fanouts):
    import torch
    row_ptr, col, centers = ladder_graph()
    weights = ladder_weights(cls, col.shape[0])
    g, ts = _weighted_structure(gpu_env, mt, col_dtype, weights)
    dev_centers = torch.from_numpy(centers.astype(center_dtype)).cuda()
    for m in fanouts:
        assert_ladder_classes(row_ptr, centers, m)
        o_off, o_ids, o_lid, o_egid = weighted_reference(cls, m)          # (asserts that the oracle's keys hold no NaN)
        off, ids, lid, egid = g.weighted_sample_without_replacement_one_hop(
            "w", dev_centers, m, random_seed=weighted_seed(m), need_center_local_output=True, need_edge_output=True)
        off, ids, lid, egid = [t.cpu().numpy() for t in (off, ids, lid, egid)]
        assert np.array_equal(off, o_off), "offsets differ at max_sample_count=%d" % m
        assert_sample_structure(row_ptr, centers, m, off, egid)
        if cls in ("zeros", "half_zero"):
            assert_zero_weight_order(row_ptr, centers, weights, m, off, egid)
        assert np.array_equal(egid, o_egid), "edge ids differ at max_sample_count=%d" % m
        assert np.array_equal(ids, o_ids.astype(col_dtype)), "ids differ at max_sample_count=%d" % m
        assert np.array_equal(lid, o_lid), "centre local ids differ at max_sample_count=%d" % m
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ the routes on the same kernels
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("cls", ["half_zero", "extremes32"])
def test_fused_hop_and_chain_on_degenerate_weights(gpu_env, cls, id_dtype):
    """the fused weighted hop = sampler + append_unique, the weighted one-call chain over two hops = hop by hop, at fan-outs 30
    (the register kernel with two centres per wave) and 65 (the LDS candidate list)"""
    import torch
    import wholegraph_amd.torch.graph_ops as gops
    import wholegraph_amd.torch.wholegraph_ops as wops
    from test_weighted_chain_gpu import _assert_same, _hand_rolled
    row_ptr, col, centers = ladder_graph()
    weights = ladder_weights(cls, col.shape[0])
    g, ts = _weighted_structure(gpu_env, "chunked", id_dtype, weights)
    csr = (ts[0].wmb_tensor, ts[1].wmb_tensor)
    frontier = torch.from_numpy(centers.astype(id_dtype)).cuda()
    for m in (30, 65):
        assert_ladder_classes(row_ptr, centers, m)
        seed = weighted_seed(m)
        fused = wops.sample_append_unique(*csr, frontier, m, seed, wm_csr_weight_ptr_tensor=ts[2].wmb_tensor)
        assert fused is not None, "the weighted fused hop was declined at max_sample_count=%d" % m
        off, ids, lid, egid = g.weighted_sample_without_replacement_one_hop(
            "w", frontier, m, random_seed=seed, need_center_local_output=True, need_edge_output=True)
        assert np.array_equal(egid.cpu().numpy(), weighted_reference(cls, m)[3])       # and the sampler is the oracle's
        uniq, pos = gops.append_unique(frontier, ids, need_neighbor_raw_to_unique=True)
        for name, a, b in zip(("offsets", "unique", "neighbor_pos", "center_lid"), fused, (off, uniq, pos, lid)):
            assert a.dtype == b.dtype and torch.equal(a, b), "%s differs at max_sample_count=%d" % (name, m)
        # two hops in one library call (the chain must take them: None would mean hop by hop on both sides)
        seeds = frontier[:101]
        hop_seeds = [seed, seed + 11]
        chain = wops.multilayer_sample(*csr, seeds, [m, m], hop_seeds, wm_csr_weight_ptr_tensor=ts[2].wmb_tensor)
        assert chain is not None, "the weighted chain was declined at max_sample_count=%d" % m
        got = g.multilayer_sample_without_replacement(seeds, [m, m], weight_name="w", random_seeds=hop_seeds)
        torch.cuda.synchronize()
        _assert_same(got, _hand_rolled(g, seeds, [m, m], hop_seeds))
    _destroy(ts)


# ------------------------------------------------------------------------------------------------ the first pick follows the weights
FIRST_PICK_WEIGHTS = np.array([1, 2, 3, 4, 5, 6, 7, 12], dtype=np.float32)
FIRST_PICK_NODES, FIRST_PICK_DEGREE = 8000, 320
FIRST_PICK_SEEDS = (424242, 7)


def first_pick_graph():
    """8000 nodes with the same 320 neighbours 0 .. 319, weights the pattern [1, 2, 3, 4, 5, 6, 7, 12] tiled: neighbour id % 8
    names the weight"""
    n, d = FIRST_PICK_NODES, FIRST_PICK_DEGREE
    row_ptr = np.arange(0, (n + 1) * d, d, dtype=np.int64)
    col = np.tile(np.arange(d, dtype=np.int32), n)
    weights = np.tile(FIRST_PICK_WEIGHTS, n * d // 8)
    return row_ptr, col, weights


def first_pick_chi_square(ids, m):
    """The output is key-descending, so position 0 is the neighbour of the largest key: neighbour i with probability
    w_i / sum(w) whatever M is. Chi-square of the 8 weight bins of ids[:, 0] against 8000 * w / sum(w) (7 degrees of
    freedom); also every row's M ids are distinct."""
    ids = ids.reshape(FIRST_PICK_NODES, m)
    assert np.all(np.diff(np.sort(ids, axis=1), axis=1) > 0), "a neighbour sampled twice"
    counts = np.bincount(ids[:, 0] % 8, minlength=8).astype(np.float64)
    expect = FIRST_PICK_NODES * FIRST_PICK_WEIGHTS.astype(np.float64) / FIRST_PICK_WEIGHTS.sum()
    return float(((counts - expect) ** 2 / expect).sum())


@pytest.mark.parametrize("m", [20, 40, 100, 300])       # G = 32, G = 64, the list with 128 and with 256 virtual threads
def test_first_pick_follows_the_weights(gpu_env, m):
    import torch
    import wholegraph_amd.torch.wholegraph_ops as wops
    from wholegraph_amd.torch.wholegraph_env import wrap_torch_tensor
    hold = [torch.from_numpy(a).cuda() for a in first_pick_graph()]
    wr, wc, ww = [wrap_torch_tensor(t) for t in hold]
    centers = torch.arange(FIRST_PICK_NODES, device="cuda", dtype=torch.int32)
    for seed in FIRST_PICK_SEEDS:
        off, ids = wops.weighted_sample_without_replacement(wr.handle, wc.handle, ww.handle, centers, m, seed)
        assert off[-1].item() == FIRST_PICK_NODES * m
        chi2 = first_pick_chi_square(ids.cpu().numpy(), m)
        print("first pick, max_sample_count %d, seed %d: chi-square %.2f over 7 dof" % (m, seed, chi2))
        assert chi2 < 40.0, "chi-square %.1f over 7 dof at max_sample_count=%d, seed %d" % (chi2, m, seed)   # p ~ 1e-6
