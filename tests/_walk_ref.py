"""Random walks as include/wholememory/wholegraph_amd_ext.h section 2m defines them, restated in plain Python: the reference of
tests/test_walk_streams.py (against the host/device header csrc/pcg.hpp) and of tests/test_walk_gpu.py (against the kernels).
The generator is the oracle's (oracle.pcg_raw), the logarithm of the weighted key the oracle's det_log2_1p; the key is formed
with numpy.float32 operations in the order csrc/pcg.hpp: weighted_sample_key uses. Also the ladder graph and the star graph
of the GPU tests, whose reference walks are computed once and shared."""
import numpy as np

import oracle

MASK = (1 << 64) - 1
F32 = np.float32


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def stream(seed, a, b, n):
    """the first n 32-bit outputs of stream(seed, a, b) = pcg32 init(mix(mix(seed + a) + b), subsequence a, offset 0)"""
    a &= MASK
    return oracle.pcg_raw(mix((mix((seed + a) & MASK) + b) & MASK), a, 0, n)


def weighted_key(seed, a, b, weight32):
    """A-Res key log2(u) * (1 / weight) from the draws of stream(seed, a, b)"""
    draws = stream(seed, a, b, 3)
    u0 = F32(int(draws[0]) >> 8) / F32(1 << 24)
    m = F32(-(0.5 + 0.5 * float(u0)))
    redraws = 0
    bits = int(draws[1]) | (int(draws[2]) << 32)
    while bits == 0:
        redraws += 1
        draws = stream(seed, a, b, 3 + 2 * redraws)
        bits = int(draws[-2]) | (int(draws[-1]) << 32)
    zeros = 64 - bits.bit_length() + 64 * redraws
    log2u = F32(oracle.det_log2_1p(float(m) * 2.0 ** -zeros))
    with np.errstate(all="ignore"):
        return log2u * (F32(1.0) / F32(weight32))


def _walks(row_ptr, col, starts, length, pick):
    """pick(w, t, s, deg) -> neighbour index or -1"""
    n_nodes, n = row_ptr.shape[0] - 1, starts.shape[0]
    walks = np.full((n, length + 1), -1, dtype=np.int64)
    eids = np.full((n, length), -1, dtype=np.int64)
    for w in range(n):
        v = int(starts[w])
        if not 0 <= v < n_nodes:
            continue
        walks[w, 0] = v
        for t in range(length):
            s, deg = int(row_ptr[v]), int(row_ptr[v + 1]) - int(row_ptr[v])
            if deg <= 0 or deg >= 1 << 31:
                break
            k = pick(w, t, s, deg)
            if k < 0:
                break
            c = int(col[s + k])
            if not 0 <= c < n_nodes:
                break
            walks[w, t + 1], eids[w, t] = c, s + k
            v = c
    return walks, eids


def uniform_walks(row_ptr, col, starts, length, seed):
    """-> walks int64 [n, length + 1], edge_ids int64 [n, length]"""
    draws = {}

    def pick(w, t, s, deg):
        if w not in draws:
            draws[w] = stream(seed, w, 0, length)
        return (int(draws[w][t]) * deg) >> 32
    return _walks(row_ptr, col, starts, length, pick)


def weighted_walks(row_ptr, col, weights, starts, length, seed):
    with np.errstate(all="ignore"):
        w32 = np.asarray(weights).astype(F32)

    def pick(w, t, s, deg):
        best_key, best = None, -1
        for j in range(deg):
            wt = w32[s + j]
            if not wt > 0:          # zero, negative and NaN weights are never chosen
                continue
            key = weighted_key(seed, w * length + t, j + 1, wt)
            if best < 0 or key > best_key:
                best_key, best = key, j
        return best
    return _walks(row_ptr, col, starts, length, pick)


# ------------------------------------------------------------------------------------------------ the ladder graph
LADDER_NODES, LADDER_LENGTH, LADDER_SEED = 2000, 6, 99
LADDER_HEAVY = ((7, 5000), (8, 1024), (9, 1025), (10, 63), (11, 64), (12, 0), (13, 1), (14, 65), (15, 2))
_CACHE = {}


def ladder():
    """-> row_ptr int64, col int64, weights float32, starts int64 [512] (read-only, shared). make_csr(2000, 12, 123) with
    the degrees of LADDER_HEAVY at nodes 7 .. 15, every 5th col_ind entry (entries 4, 9, ...) redirected to those nine nodes
    in turn; weights uniform in [0.05, 1.05), a tenth of them 0, node 15's two weights 0 and -1; starts 0 .. 19, then -1, 2000
    and 2005 (refused), then 489 drawn nodes."""
    if "ladder" not in _CACHE:
        from test_graph_oracle import make_csr
        row_ptr, col = make_csr(LADDER_NODES, 12, 123, heavy=list(LADDER_HEAVY))
        heavy_nodes = np.array([node for node, _ in LADDER_HEAVY], dtype=np.int64)
        redirected = np.arange(4, col.shape[0], 5)
        col[redirected] = heavy_nodes[np.arange(redirected.shape[0]) % heavy_nodes.shape[0]]
        rng = np.random.default_rng(7)
        weights = (rng.random(col.shape[0]) + 0.05).astype(F32)
        weights[rng.random(col.shape[0]) < 0.1] = 0.0
        weights[row_ptr[15]:row_ptr[16]] = (0.0, -1.0)
        starts = np.concatenate([np.arange(20), [-1, LADDER_NODES, LADDER_NODES + 5],
                                 np.random.default_rng(5).integers(0, LADDER_NODES, 489)]).astype(np.int64)
        assert starts.shape[0] == 512
        for a in (row_ptr, col, weights, starts):
            a.setflags(write=False)
        _CACHE["ladder"] = (row_ptr, col, weights, starts)
    return _CACHE["ladder"]


def ladder_uniform(length=LADDER_LENGTH):
    key = ("uniform", length)
    if key not in _CACHE:
        row_ptr, col, _, starts = ladder()
        _CACHE[key] = uniform_walks(row_ptr, col, starts, length, LADDER_SEED)
    return _CACHE[key]


def ladder_weighted():
    if "weighted" not in _CACHE:
        row_ptr, col, weights, starts = ladder()
        _CACHE["weighted"] = weighted_walks(row_ptr, col, weights, starts, LADDER_LENGTH, LADDER_SEED)
    return _CACHE["weighted"]


def ladder_measures(walks, eids):
    """what the ladder must exercise: steps taken from nodes with at least 63 neighbours, steps from the 5000-neighbour node,
    walks ending at node 12 (no neighbours) and at node 15 (no eligible neighbour), start nodes refused"""
    row_ptr = ladder()[0]
    taken = eids >= 0
    src = walks[:, :-1][taken]
    deg = row_ptr[src + 1] - row_ptr[src]
    last = np.array([row[row >= 0][-1] if (row >= 0).any() else -1 for row in walks])
    ended = ~taken[:, -1]          # the last step was not taken: the walk ended at `last`
    return {"from_big": int((deg >= 63).sum()), "from_5000": int((src == 7).sum()),
            "end_at_12": int((ended & (last == 12)).sum()), "end_at_15": int((ended & (last == 15)).sum()),
            "refused": int((walks[:, 0] < 0).sum())}


def assert_ladder_measures():
    """lower bounds on the REFERENCE walks, so that a later change of the graph cannot empty a case"""
    u, w = ladder_measures(*ladder_uniform()), ladder_measures(*ladder_weighted())
    for m in (u, w):
        assert m["from_big"] >= 200 and m["from_5000"] >= 30 and m["end_at_12"] >= 40 and m["refused"] == 3, (u, w)
    assert w["end_at_15"] >= 30, w
    return u, w


# ------------------------------------------------------------------------------------------------ the star graph
STAR_WEIGHTS = np.arange(1, 9, dtype=F32)
STAR_WALKS, STAR_LENGTH, STAR_SEED = 8000, 5, 1


def star():
    """node 0 has the 8 neighbours 1 .. 8 with weights 1 .. 8, every leaf points back at node 0"""
    row_ptr = np.concatenate([[0], np.arange(8, 17)]).astype(np.int64)
    col = np.concatenate([np.arange(1, 9), np.zeros(8, dtype=np.int64)]).astype(np.int64)
    weights = np.concatenate([STAR_WEIGHTS, np.ones(8, dtype=F32)])
    return row_ptr, col, weights


def star_statistics(walks, weighted):
    """-> (largest goodness-of-fit chi-square of columns 1, 3, 5 over 7 degrees of freedom, largest independence chi-square
    over 49 of the 8 x 8 tables of columns (1, 3), (3, 5) and of walks w against w + s for s in 1, 2, 64, 1024)"""
    walks = np.asarray(walks, dtype=np.int64)
    n = walks.shape[0]
    assert np.all(walks[:, [0, 2, 4]] == 0), "columns 0, 2 and 4 of every walk must be node 0"
    picks = walks[:, [1, 3, 5]] - 1
    assert picks.min() >= 0 and picks.max() <= 7
    p = (STAR_WEIGHTS / STAR_WEIGHTS.sum()).astype(np.float64) if weighted else np.full(8, 0.125)
    fit = max(float(((np.bincount(picks[:, c], minlength=8) - n * p) ** 2 / (n * p)).sum()) for c in range(3))

    def independence(x, y):
        table = np.zeros((8, 8))
        np.add.at(table, (x, y), 1)
        expect = np.outer(table.sum(1), table.sum(0)) / table.sum()
        return float(((table - expect) ** 2 / expect).sum())
    tables = [independence(picks[:, 0], picks[:, 1]), independence(picks[:, 1], picks[:, 2])]
    for s in (1, 2, 64, 1024):
        tables += [independence(picks[:-s, c], picks[s:, c]) for c in range(3)]
    return fit, max(tables)
