"""node2vec (p, q) walks as include/wholememory/wholegraph_amd_ext.h section 2n defines them, restated in plain Python: the
reference of tests/test_n2v_streams.py (against the host/device header csrc/walk_n2v.hpp) and of tests/test_n2v_gpu.py (against
the kernels). Streams, keys and the walk loop are tests/_walk_ref.py's; the effective weight is formed with numpy.float32 and
"x occurs in the previous node's row" is asked of a Python set per row. Also the graphs of the GPU tests — the clustered ladder,
its unsorted twin, the kite — whose reference walks are computed once and shared."""
import numpy as np

import _walk_ref as wref

F32 = np.float32
_LOG2U = {}
_CACHE = {}


def log2u(seed, a, b):
    """log2(u) of stream(seed, a, b): _walk_ref.weighted_key with weight 1.0f is log2(u) * (1.0f / 1.0f) = log2(u), bit for
    bit. It does not depend on p, q or the graph, so it is kept across the reference runs."""
    k = (seed, a, b)
    if k not in _LOG2U:
        _LOG2U[k] = wref.weighted_key(seed, a, b, F32(1.0))
    return _LOG2U[k]


def node2vec_walks(row_ptr, col, weights, starts, length, p, q, seed, first_walk=0):
    """-> walks int64 [n, length + 1], edge_ids int64 [n, length]. weights None: every edge has weight 1.0f. first_walk: the
    number of starts[0] in the batch it was cut from (walk w of the result uses the streams of walk first_walk + w)."""
    inv_p, inv_q = F32(1.0) / F32(p), F32(1.0) / F32(q)
    col = np.asarray(col)
    with np.errstate(all="ignore"):
        w32 = None if weights is None else np.asarray(weights).astype(F32)
    rows = {}
    where = {}          # walk -> [previous node or None, current node]

    def row_set(node):
        if node not in rows:
            rows[node] = set(int(x) for x in col[int(row_ptr[node]):int(row_ptr[node + 1])])
        return rows[node]

    def pick(w, t, s, deg):
        if t == 0:
            where[w] = [None, int(starts[w])]
        u, v = where[w]
        near = row_set(u) if u is not None else None
        best_key, best = None, -1
        for j in range(deg):
            x = int(col[s + j])
            a = F32(1.0) if u is None else inv_p if x == u else F32(1.0) if x in near else inv_q
            with np.errstate(all="ignore"):
                ew = (F32(1.0) if w32 is None else w32[s + j]) * a
                if not ew > 0:          # zero, negative and NaN effective weights are never chosen
                    continue
                key = log2u(seed, (first_walk + w) * length + t, j + 1) * (F32(1.0) / ew)
            if best < 0 or key > best_key:
                best_key, best = key, j
        if best >= 0:
            where[w] = [v, int(col[s + best])]
        return best
    return wref._walks(row_ptr, col, starts, length, pick)


# --------------------------------------------------------------------------------------- the clustered ladder
NODES, LENGTH, SEED = wref.LADDER_NODES, wref.LADDER_LENGTH, wref.LADDER_SEED
RING = 8
# how many nodes have 0 .. 12 neighbours: a third are leaves of one or two, most of the rest have nine or more
DEGREE_SHARE = np.array([3, 19, 4, 1, 1, 1, 1, 1, 1, 9, 15, 20, 24]) / 100.0
TWIN_CAP = 1025
PQ = ((0.25, 4.0), (4.0, 0.25), (1.0, 2.0), (2.0, 1.0), (1.0, 1.0))
PQ_MEASURED = ((0.25, 4.0), (4.0, 0.25))


def _sort_rows(row_ptr, col, weights):
    for v in range(row_ptr.shape[0] - 1):
        s, e = int(row_ptr[v]), int(row_ptr[v + 1])
        o = np.argsort(col[s:e], kind="stable")
        col[s:e], weights[s:e] = col[s:e][o], weights[s:e][o]


def clustered_ladder(heavy=True):
    """-> row_ptr int64, col int64, weights float32, starts int64 [512] (read-only, shared). 2000 nodes on a ring; a node has
    0 .. 12 neighbours at ring distance <= 8, so that consecutive nodes share neighbours; nodes 7 .. 15 have the degrees of
    _walk_ref.LADDER_HEAVY (their neighbours drawn from the whole graph) and every 5th col_ind entry is redirected to those
    nine in turn; weights and starts as _walk_ref.ladder(); every row ascending, its weights carried along. heavy=False: the
    same construction without the heavy degrees and without the redirection (the graph of the large batch)."""
    key = ("ladder", heavy)
    if key not in _CACHE:
        rng = np.random.default_rng(123)
        deg = rng.choice(13, NODES, p=DEGREE_SHARE)
        if heavy:
            for node, d in wref.LADDER_HEAVY:
                deg[node] = d
        row_ptr = np.zeros(NODES + 1, dtype=np.int64)
        np.cumsum(deg, out=row_ptr[1:])
        src = np.repeat(np.arange(NODES), deg)
        ring = np.concatenate([np.arange(-RING, 0), np.arange(1, RING + 1)])
        col = np.zeros(src.shape[0], dtype=np.int64)
        core = (deg >= 3) & (deg <= 12)
        for v in np.flatnonzero(core):   # distinct neighbours, so that the rows of two nearby nodes overlap in many entries
            near = (v + rng.permutation(ring)) % NODES
            near = near[core[near]] if core[near].any() else near
            col[row_ptr[v]:row_ptr[v + 1]] = np.resize(near, deg[v])      # (a short list is repeated: parallel edges)
        locked = np.zeros(src.shape[0], dtype=bool)

        def point_back(x, v, lock):
            """one entry of core node x's row becomes v (an entry that is not locked)"""
            free = np.flatnonzero(~locked[row_ptr[x]:row_ptr[x + 1]])
            if core[x] and free.shape[0] > 0:
                e = row_ptr[x] + free[rng.integers(0, free.shape[0])]
                col[e], locked[e] = v, lock
        # a node of one neighbour pairs up with another such node nearby, each the other's only neighbour (a walk that enters the
        # pair only ever returns), or else hangs on a nearby node of many neighbours as a leaf; a node of two neighbours hangs on
        # a nearby node and on one of that node's neighbours, and closes a triangle
        paired = np.zeros(NODES, dtype=bool)
        for v in np.flatnonzero((deg >= 1) & (deg <= 2)):
            if paired[v]:
                continue
            around = (v + rng.permutation(ring)) % NODES
            mates = [int(x) for x in around if deg[x] == 1 and not paired[x] and not 7 <= x <= 15]
            near = [int(x) for x in around if core[x]] or [int((v + 1) % NODES)]
            if deg[v] == 1 and mates and not 7 <= v <= 15:
                col[row_ptr[v]], col[row_ptr[mates[0]]] = mates[0], v
                paired[v] = paired[mates[0]] = True
                continue
            picks = near[:1]
            if deg[v] == 2:
                row = col[row_ptr[near[0]]:row_ptr[near[0] + 1]]
                second = [int(x) for x in row if core[x] and x != near[0] and min((x - v) % NODES, (v - x) % NODES) <= RING]
                picks.append(second[0] if second else near[-1])
            col[row_ptr[v]:row_ptr[v + 1]] = picks
            for x in picks:
                point_back(x, int(v), True)
        if heavy:
            far = rng.integers(0, NODES, src.shape[0])
            is_heavy = np.isin(src, [node for node, d in wref.LADDER_HEAVY if d > 12])
            col[is_heavy] = far[is_heavy]
            heavy_nodes = np.array([node for node, _ in wref.LADDER_HEAVY], dtype=np.int64)
            redirected = np.arange(4, col.shape[0], 5)
            col[redirected] = heavy_nodes[np.arange(redirected.shape[0]) % heavy_nodes.shape[0]]
        wrng = np.random.default_rng(7)
        weights = (wrng.random(col.shape[0]) + 0.05).astype(F32)
        weights[wrng.random(col.shape[0]) < 0.1] = 0.0
        _sort_rows(row_ptr, col, weights)
        if heavy:
            weights[row_ptr[15]:row_ptr[16]] = (0.0, -1.0)
        starts = np.array(wref.ladder()[3])
        for a in (row_ptr, col, weights, starts):
            a.setflags(write=False)
        _CACHE[key] = (row_ptr, col, weights, starts)
    return _CACHE[key]


def unsorted_twin():
    """the clustered ladder with the heavy rows cut to TWIN_CAP entries and every row permuted by a fixed generator, its
    weights carried along -> row_ptr, col, weights, starts"""
    if "twin" not in _CACHE:
        row_ptr, col, weights, starts = clustered_ladder()
        rng = np.random.default_rng(2024)
        cols, wgts, new_ptr = [], [], [0]
        for v in range(NODES):
            s, e = int(row_ptr[v]), min(int(row_ptr[v + 1]), int(row_ptr[v]) + TWIN_CAP)
            o = rng.permutation(e - s)
            cols.append(col[s:e][o]), wgts.append(weights[s:e][o])
            new_ptr.append(new_ptr[-1] + e - s)
        out = (np.array(new_ptr, dtype=np.int64), np.concatenate(cols), np.concatenate(wgts), starts)
        for a in out:
            a.setflags(write=False)
        _CACHE["twin"] = out
    return _CACHE["twin"]


def ladder_walks(p, q, weighted, twin=False):
    key = ("walks", float(p), float(q), bool(weighted), bool(twin))
    if key not in _CACHE:
        row_ptr, col, weights, starts = unsorted_twin() if twin else clustered_ladder()
        _CACHE[key] = node2vec_walks(row_ptr, col, weights if weighted else None, starts, LENGTH, p, q, SEED)
    return _CACHE[key]


def ladder_measures(walks, eids, graph):
    """what the clustered ladder must exercise, counted over the steps t >= 1 that were taken: returns (x == u), steps to a
    neighbour of u, steps to neither, steps from a row that held all three classes, steps from the 5000-neighbour node; and
    walks that ended at node 15, which has no eligible neighbour"""
    row_ptr, col = graph[0], graph[1]
    rows = {}

    def row_set(node):
        if node not in rows:
            rows[node] = set(int(x) for x in col[int(row_ptr[node]):int(row_ptr[node + 1])])
        return rows[node]
    m = dict(returns=0, to_near=0, to_far=0, from_mixed=0, from_5000=0)
    for w in range(walks.shape[0]):
        for t in range(1, eids.shape[1]):
            if eids[w, t] < 0:
                break
            u, v, x = int(walks[w, t - 1]), int(walks[w, t]), int(walks[w, t + 1])
            near = row_set(u)
            m["returns" if x == u else "to_near" if x in near else "to_far"] += 1
            mine = row_set(v)
            m["from_mixed"] += int(u in mine and any(y != u and y in near for y in mine) and
                                   any(y != u and y not in near for y in mine))
            m["from_5000"] += int(v == 7)
    last = np.array([row[row >= 0][-1] if (row >= 0).any() else -1 for row in walks])
    m["end_at_15"] = int(((eids[:, -1] < 0) & (last == 15)).sum())
    return m


def assert_ladder_measures():
    """lower bounds on the REFERENCE walks (weighted, sorted graph), so that a later change of the graph cannot empty a case"""
    graph = clustered_ladder()
    plain = ladder_walks(1.0, 1.0, True)[0]
    out = {}
    for p, q in PQ_MEASURED:
        walks, eids = ladder_walks(p, q, True)
        m = ladder_measures(walks, eids, graph)
        m["differ_from_plain"] = int((walks != plain).any(axis=1).sum())
        out[(p, q)] = m
        assert min(m["returns"], m["to_near"], m["to_far"], m["from_mixed"]) >= 200, out
        assert m["from_5000"] >= 30 and m["end_at_15"] >= 30 and m["differ_from_plain"] >= 256, out
    return out


# ------------------------------------------------------------------------------------------------ the kite
KITE_WALKS, KITE_LENGTH, KITE_P, KITE_Q = 24000, 2, 0.5, 2.0
KITE_WEIGHTS = np.arange(1, 7, dtype=F32)


def kite():
    """node 1 has the row [0, 2, 3], node 0 the row [1, 2, 3, 4, 5, 6] (weights 1 .. 6 in the weighted form), nodes 2 .. 6 the
    row [0]. A walk 1 -> 0 -> x meets every class: x = 1 returns, 2 and 3 are neighbours of node 1, 4 .. 6 are neither."""
    row_ptr = np.array([0, 6, 9, 10, 11, 12, 13, 14], dtype=np.int64)
    col = np.array([1, 2, 3, 4, 5, 6, 0, 2, 3, 0, 0, 0, 0, 0], dtype=np.int64)
    weights = np.ones(col.shape[0], dtype=F32)
    weights[:6] = KITE_WEIGHTS
    return row_ptr, col, weights


def kite_statistic(walks, weighted):
    """chi-square over 5 degrees of freedom of column 2 among the walks whose column 1 is node 0, against
    {1: 1 / p; 2, 3: 1; 4, 5, 6: 1 / q} (times the weights 1 .. 6 in the weighted form), normalised"""
    walks = np.asarray(walks, dtype=np.int64)
    assert walks.shape == (KITE_WALKS, KITE_LENGTH + 1) and np.all(walks[:, 0] == 1)
    through = walks[walks[:, 1] == 0]
    assert KITE_WALKS // 4 < through.shape[0] < KITE_WALKS // 2, through.shape     # about a third
    assert through[:, 2].min() >= 1 and through[:, 2].max() <= 6
    bias = np.array([1 / KITE_P, 1, 1, 1 / KITE_Q, 1 / KITE_Q, 1 / KITE_Q])
    expect = bias * (KITE_WEIGHTS.astype(np.float64) if weighted else 1.0)
    expect = expect / expect.sum() * through.shape[0]
    counts = np.bincount(through[:, 2] - 1, minlength=6)
    return float(((counts - expect) ** 2 / expect).sum())


# the seed was fixed before the values were computed (tests/test_n2v_streams.py computes them with the host program; the
# kernel walks the same walks, so tests/test_n2v_gpu.py asks for the same values; DESIGN.md 3.18 states them)
KITE_SEED = 1
KITE_CHI2 = {False: 2.598877046060145, True: 5.2498561942223745}
