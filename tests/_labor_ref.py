"""LABOR layer-neighbour sampling as include/wholememory/wholegraph_amd_ext.h section 2v defines it, restated in numpy on
tests/_walk_ref.stream, and the LABOR ladder: the reference of tests/test_labor_gpu.py, computed once per case and shared."""
import numpy as np

from _tsample_ref import row_valid
from _walk_ref import MASK, stream

_U64 = np.uint64
LADDER_SEED = 2023
# nodes 0 .. 21: 0, 1 and M - 1, M, M + 1 for every M the tests use, then 129 and 1000 neighbours; node 22: 40 entries over 6 ids
LADDER_DEGREES = (0, 1, 2, 4, 5, 6, 9, 10, 11, 31, 32, 33, 34, 63, 64, 65, 99, 100, 101, 129, 1000, 3, 40)
_CACHE = {}


def variate(seed, c):
    """v(c): the first 32-bit output of stream(seed, (uint64)c, 0)"""
    return int(stream(seed, int(c) & MASK, 0, 1)[0])


def variates(seed, ids):
    """the same for an array of node ids: PCG-XSH-RR 64/32 after init(mix(mix(seed + c)), subsequence c, offset 0) -> uint64"""
    a = np.asarray(ids, dtype=np.int64).astype(_U64)      # (sign-extended)
    with np.errstate(over="ignore"):
        def vmix(z):
            z = z + _U64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
            return z ^ (z >> _U64(31))
        inc = (a << _U64(1)) | _U64(1)
        old = (inc + vmix(vmix(_U64(seed & MASK) + a))) * _U64(6364136223846793005) + inc
        xorshifted = (((old >> _U64(18)) ^ old) >> _U64(27)) & _U64(0xFFFFFFFF)
        rot = old >> _U64(59)
        return ((xorshifted >> rot) | (xorshifted << ((_U64(32) - rot) & _U64(31)))) & _U64(0xFFFFFFFF)


def kept_positions(ids, m, mode, seed):
    """the positions j of a row (its col_ind entries `ids`) that centre keeps, ascending"""
    n = len(ids)
    v = variates(seed, ids)
    if mode == "poisson":
        assert 1 <= m < 1 << 31
        return np.nonzero(v * _U64(n) < _U64(m << 32))[0]      # (both sides below 2^63)
    assert m <= 64
    if m <= 0 or n <= m:
        return np.arange(n)
    return np.sort(np.lexsort((np.arange(n), v))[:m])      # the smallest v, ties to the lowest j


def labor_sample(row_ptr, col, centers, m, mode="fixed", seed=0):
    """-> offsets int32 [n + 1], ids (col's dtype), center local id int32, edge id int64"""
    n_nodes, n_edges = len(row_ptr) - 1, len(col)
    counts, egid = [], []
    for u in (int(x) for x in centers):
        s = e = 0
        if 0 <= u < n_nodes and row_valid(int(row_ptr[u]), int(row_ptr[u + 1]), n_edges):
            s, e = int(row_ptr[u]), int(row_ptr[u + 1])
        egid.append(s + kept_positions(col[s:e], m, mode, seed))
        counts.append(len(egid[-1]))
    egid = np.concatenate(egid + [np.empty(0, np.int64)]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return offsets, np.asarray(col)[egid], np.repeat(np.arange(len(counts)), counts).astype(np.int32), egid


def tiled(sample, n_base, reps):
    """the sample of np.tile(centres, reps) from the sample of the n_base centres: a row depends on its node alone"""
    offsets, ids, lid, egid = sample
    lids = (lid[None, :] + (np.arange(reps) * n_base)[:, None]).reshape(-1).astype(np.int32)
    counts = np.tile(np.diff(offsets), reps)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), np.tile(ids, reps), lids, np.tile(egid, reps)


def labor_ladder():
    """-> row_ptr int64 [303], col int64, centres int64 (read-only, shared). 302 nodes: LADDER_DEGREES at nodes 0 .. 22, then 0 .. 8
    neighbours; entries drawn from the 300 good nodes, every 4th one node 7; node 22 has multi-edges; node 300 has s > e and
    node 301 e > n_edges. The centres: every node in a shuffled order, -1, n_nodes, and nodes 20 and 22 a second time."""
    if "ladder" not in _CACHE:
        rng = np.random.default_rng(11)
        degrees = np.concatenate([LADDER_DEGREES, rng.integers(0, 9, 300 - len(LADDER_DEGREES))])
        row_ptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
        col = rng.integers(0, 300, row_ptr[-1]).astype(np.int64)
        col[::4] = 7
        col[row_ptr[22]:row_ptr[23]] = rng.choice(300, 6, replace=False)[rng.integers(0, 6, 40)]
        row_ptr = np.concatenate([row_ptr, [row_ptr[-1] - 3, row_ptr[-1] + 5]])
        centres = np.concatenate([rng.permutation(302), [-1, 302, 20, 22]]).astype(np.int64)
        for a in (row_ptr, col, centres):
            a.setflags(write=False)
        _CACHE["ladder"] = (row_ptr, col, centres)
        # the cases the Poisson rule must meet on this graph under LADDER_SEED, on the REFERENCE: with N > M nobody, some, all
        c, n = np.diff(ladder_sample(1, "poisson")[0]), np.diff(ladder_sample(-1, "fixed")[0])
        assert ((n > 1) & (c == 0)).any() and ((n > 1) & (c > 0) & (c < n)).any() and ((n > 1) & (c == n)).any()
    return _CACHE["ladder"]


def ladder_sample(m, mode):
    """the reference outputs on the ladder's centres"""
    if (m, mode) not in _CACHE:
        _CACHE[(m, mode)] = labor_sample(*labor_ladder(), m, mode, LADDER_SEED)
    return _CACHE[(m, mode)]
