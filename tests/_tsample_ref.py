"""Temporal neighbour sampling as include/wholememory/wholegraph_amd_ext.h section 2r defines it, restated in plain Python: the
reference of tests/test_tsample_streams.py (against the host/device header csrc/tsample.hpp) and of tests/test_tsample_gpu.py
(against the kernels of csrc/kernels/tsample.hip). The draws come from tests/_walk_ref.stream; times and the unsigned window
are Python integers. `fast_draws` restates the same stream over a whole row in numpy (for the 70 001-centre batch alone); the
two are asserted equal in tests/test_tsample_streams.py. Also the temporal ladder, the octet of the uniformity test and their
measures; reference outputs are computed once and shared."""
import numpy as np

from _walk_ref import MASK, ladder, mix, stream

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
STRATEGIES = {"uniform": 0, "last": 1}
_CACHE = {}
_U64 = np.uint64


def row_valid(s, e, n_edges):
    """the damaged-graph rule of sections 2o and 2q: bounds that are a row"""
    return 0 <= s <= e <= n_edges and e - s < (1 << 31)


def eligible(ts, t, inclusive, window):
    """window None or < 0: none"""
    if ts > t or (not inclusive and ts == t):
        return False
    if window is None or window < 0:
        return True
    return ((t & MASK) - (ts & MASK)) & MASK <= window


def draws(seed, i, js):
    """r(i, j) for the positions js: the first 32-bit output of stream(seed, i, j + 1)"""
    return [int(stream(seed, i, j + 1, 1)[0]) for j in js]


def fast_draws(seed, i, js):
    """the same numbers from numpy: PCG-XSH-RR 64/32 after init(mix(mix(seed + i) + j + 1), subsequence i, offset 0)"""
    js = np.asarray(js, dtype=_U64)
    with np.errstate(over="ignore"):
        def vmix(z):
            z = z + _U64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
            return z ^ (z >> _U64(31))
        a = i & MASK
        seeded = vmix(_U64(mix((seed + a) & MASK)) + js + _U64(1))
        inc = _U64(((a << 1) | 1) & MASK)
        # state = 0; step; state += seed; step: the first output is made from the state the second step leaves
        old = (inc + seeded) * _U64(6364136223846793005) + inc
        xorshifted = (((old >> _U64(18)) ^ old) >> _U64(27)) & _U64(0xFFFFFFFF)
        rot = old >> _U64(59)
        out = ((xorshifted >> rot) | (xorshifted << ((_U64(32) - rot) & _U64(31)))) & _U64(0xFFFFFFFF)
    return [int(x) for x in out]


def select(js, keys, m):
    """the m positions with the largest key, ties to the lowest position, in ascending position"""
    order = sorted(range(len(js)), key=lambda k: (-keys[k], js[k]))
    return sorted(js[k] for k in order[:m])


def temporal_sample(row_ptr, col, edge_time, centers, center_times, max_sample_count, strategy="uniform", inclusive=True,
                    time_window=None, seed=0, first_center=0, draw=draws, eligible_counts=None):
    """-> offsets int32 [n + 1], ids (col's dtype), center local id int32, edge id int64. Centre k of this call is centre
    first_center + k of the batch. eligible_counts: a list that receives E_i of every centre"""
    n_nodes, n_edges = len(row_ptr) - 1, len(col)
    assert len(edge_time) == n_edges and len(center_times) == len(centers) and max_sample_count <= 64
    code = STRATEGIES[strategy]
    offsets, lid, egid = [0], [], []
    for k, (u, t) in enumerate(zip((int(x) for x in centers), (int(x) for x in center_times))):
        js = []
        if 0 <= u < n_nodes:
            s, e = int(row_ptr[u]), int(row_ptr[u + 1])
            if row_valid(s, e, n_edges):
                js = [j for j in range(e - s) if eligible(int(edge_time[s + j]), t, inclusive, time_window)]
        if eligible_counts is not None:
            eligible_counts.append(len(js))
        if 0 < max_sample_count < len(js):
            keys = draw(seed, first_center + k, js) if code == 0 else [int(edge_time[s + j]) for j in js]
            js = select(js, keys, max_sample_count)
        lid += [k] * len(js)
        egid += [s + j for j in js]
        offsets.append(len(egid))
    assert offsets[-1] < 1 << 31
    egid = np.array(egid, dtype=np.int64)
    return np.array(offsets, dtype=np.int32), np.asarray(col)[egid], np.array(lid, dtype=np.int32), egid


# ------------------------------------------------------------------------------------------------ the temporal ladder
LADDER_SEED = 2718
LADDER_M = 32
SPECIAL_CENTRES = ((13, INT64_MIN), (14, INT64_MAX), (15, 0))      # batch position -> centre time


def temporal_ladder():
    """-> row_ptr, col, edge_time int64 [n_edges], starts int64 [512], center_times int64 [512] (read-only, shared). The graph
    and batch of _walk_ref.ladder(); edge times default_rng(77).integers(0, 1000, n_edges) with four rows overridden: node 8
    (1024 neighbours) all one value, 10 before the time of batch position 8; node 9 (1025) ascending, entry 32 equal to the
    time of batch position 9, so that that centre has 33 eligible neighbours and 32 earlier ones; node 10 (63) entirely later
    than every drawn centre time; node 14 (65) INT64_MIN at entries 0, 3, ... and INT64_MAX at entries 1, 4, ... Centre times
    default_rng(78).integers(0, 1000, 512) with positions 13, 14 and 15 (nodes 13, 14, 15) set to INT64_MIN, INT64_MAX and 0."""
    if "ladder" not in _CACHE:
        row_ptr, col, _, starts = ladder()
        assert starts[8] == 8 and starts[9] == 9 and starts[14] == 14
        ctimes = np.random.default_rng(78).integers(0, 1000, starts.shape[0]).astype(np.int64)
        for pos, t in SPECIAL_CENTRES:
            ctimes[pos] = t
        etime = np.random.default_rng(77).integers(0, 1000, col.shape[0]).astype(np.int64)
        etime[row_ptr[8]:row_ptr[9]] = ctimes[8] - 10
        etime[row_ptr[9]:row_ptr[10]] = ctimes[9] - 32 + np.arange(row_ptr[10] - row_ptr[9])
        etime[row_ptr[10]:row_ptr[11]] = 2000 + np.arange(row_ptr[11] - row_ptr[10])
        etime[row_ptr[14]:row_ptr[15]:3] = INT64_MIN
        etime[row_ptr[14] + 1:row_ptr[15]:3] = INT64_MAX
        for a in (etime, ctimes):
            a.setflags(write=False)
        _CACHE["ladder"] = (row_ptr, col, etime, starts, ctimes)
    return _CACHE["ladder"]


def ladder_sample(max_sample_count=LADDER_M, strategy="uniform", inclusive=True, time_window=None):
    """the reference outputs on the ladder's 512 centres, with E_i as a fifth entry"""
    key = ("sample", max_sample_count, strategy, inclusive, time_window)
    if key not in _CACHE:
        row_ptr, col, etime, starts, ctimes = temporal_ladder()
        counts = []
        out = temporal_sample(row_ptr, col, etime, starts, ctimes, max_sample_count, strategy, inclusive, time_window, LADDER_SEED,
                              draw=cached_draws, eligible_counts=counts)
        _CACHE[key] = out + (np.array(counts, dtype=np.int64),)
    return _CACHE[key]


def cached_draws(seed, i, js):
    """the ladder's draws, made once per (seed, centre, position): the configurations of the ladder share them"""
    memo = _CACHE.setdefault(("draws", seed, i), {})
    for j in js:
        if j not in memo:
            memo[j] = int(stream(seed, i, j + 1, 1)[0])
    return [memo[j] for j in js]


def tiled_ladder(n=70001):
    """the ladder batch repeated to n centres -> centres, times, reference outputs (strategy uniform, M = 32, fast_draws)"""
    key = ("tiled", n)
    if key not in _CACHE:
        row_ptr, col, etime, starts, ctimes = temporal_ladder()
        reps = (n + starts.shape[0] - 1) // starts.shape[0]
        centres, times = np.tile(starts, reps)[:n], np.tile(ctimes, reps)[:n]
        _CACHE[key] = (centres, times, temporal_sample(row_ptr, col, etime, centres, times, LADDER_M, "uniform", True, None,
                                                       LADDER_SEED, draw=fast_draws))
    return _CACHE[key]


def ladder_measures():
    """what the temporal ladder must exercise at M = 32, measured on the REFERENCE: centres by their number of eligible
    neighbours under inclusive=True — E = M itself is held under inclusive=False (`exactly_m_earlier`: batch position 9, node 9,
    which has M + 1 under inclusive=True); `exactly_m_inclusive` says whether inclusive=True holds one too —, centres whose row a
    window of 50 cuts, and centres whose
    strategy-1 selection is decided by position (the M-th and the (M + 1)-th largest eligible time are equal)"""
    row_ptr, col, etime, starts, ctimes = temporal_ladder()
    m = LADDER_M
    e_incl, e_excl, e_win = ladder_sample()[4], ladder_sample(inclusive=False)[4], ladder_sample(time_window=50)[4]
    ties = 0
    for u, t, e in zip(starts, ctimes, e_incl):
        if e > m:
            row = sorted((int(x) for x in etime[row_ptr[u]:row_ptr[u + 1]] if eligible(int(x), int(t), True, None)), reverse=True)
            ties += row[m - 1] == row[m]
    return {"none": int((e_incl == 0).sum()), "below": int(((e_incl > 0) & (e_incl < m)).sum()),
            "exactly_m_inclusive": int((e_incl == m).sum()), "exactly_m_earlier": int((e_excl == m).sum()),
            "m_plus_1": int((e_incl == m + 1).sum()),
            "above_64": int((e_incl > 64).sum()), "above_1024": int((e_incl > 1024).sum()),
            "cut_by_window": int(((e_win < e_incl) & (e_win > 0)).sum()), "emptied_by_window": int(((e_win == 0) & (e_incl > 0)).sum()),
            "position_ties": int(ties), "refused": int(((starts < 0) | (starts >= row_ptr.shape[0] - 1)).sum())}


def assert_ladder_measures():
    """lower bounds on the REFERENCE, so that a later change of the ladder cannot empty a case"""
    got = ladder_measures()
    for name in ("none", "below", "exactly_m_earlier", "m_plus_1", "above_64", "above_1024", "cut_by_window", "position_ties"):
        assert got[name] >= 1, (name, got)
    assert got["none"] >= 10 and got["below"] >= 300 and got["cut_by_window"] >= 100 and got["refused"] == 3, got
    return got


# ------------------------------------------------------------------------------------------------ the octet
OCTET_CENTRES, OCTET_TIME, OCTET_M, OCTET_SEED = 6000, 6, 2, 31415
OCTET_CHI2_SINGLE, OCTET_CHI2_PAIRS = 1.586, 7.92      # over 5 and 14 degrees of freedom; the 1 % points are 15.09 and 29.14


def octet():
    """one node with 8 neighbours whose edge times are 1 .. 8 (the neighbours point at nothing)"""
    row_ptr = np.array([0, 8] + [8] * 8, dtype=np.int64)
    col = np.arange(1, 9, dtype=np.int64)
    return row_ptr, col, np.arange(1, 9, dtype=np.int64)


def octet_sample():
    if "octet" not in _CACHE:
        row_ptr, col, etime = octet()
        _CACHE["octet"] = temporal_sample(row_ptr, col, etime, np.zeros(OCTET_CENTRES, dtype=np.int64),
                                          np.full(OCTET_CENTRES, OCTET_TIME, dtype=np.int64), OCTET_M, "uniform", True, None,
                                          OCTET_SEED)
    return _CACHE["octet"]


def octet_statistics(offsets, egid):
    """-> (chi-square of the six eligible positions' counts over 5 degrees of freedom, chi-square of the 15 pairs over 14);
    asserts that every centre has two distinct samples among positions 0 .. 5"""
    offsets, egid = np.asarray(offsets, dtype=np.int64), np.asarray(egid, dtype=np.int64)
    n = offsets.shape[0] - 1
    assert np.array_equal(offsets, 2 * np.arange(n + 1)) and egid.shape[0] == 2 * n
    pairs = egid.reshape(n, 2)
    assert pairs.min() >= 0 and pairs.max() <= 5, "positions 6 and 7 lie in the centre's future"
    assert (pairs[:, 0] < pairs[:, 1]).all()
    single = np.bincount(pairs.ravel(), minlength=6).astype(np.float64)
    chi_single = float(((single - 2 * n / 6) ** 2 / (2 * n / 6)).sum())
    table = np.zeros((6, 6))
    np.add.at(table, (pairs[:, 0], pairs[:, 1]), 1)
    counts = table[np.triu_indices(6, 1)]
    chi_pairs = float(((counts - n / 15) ** 2 / (n / 15)).sum())
    return chi_single, chi_pairs
