"""Per-relation fan-out neighbour sampling as include/wholememory/wholegraph_amd_ext.h section 2t defines it, restated in numpy
and plain Python, and the typed ladder: the reference of tests/test_tysample_gpu.py, computed once and shared. The draws come
from tests/_walk_ref.stream (`fast_draws`, asserted equal to it in tests/test_tsample_streams.py, for the 70 001 centres alone)."""
import numpy as np

from _tsample_ref import fast_draws, row_valid, select
from _walk_ref import ladder, stream

LADDER_SEED = 1618
LADDER_R = 4
LADDER_FANOUTS = (8, 8, 8, 8)
_CACHE = {}


def draws(seed, i, js):
    """r(i, j) for the positions js: the first 32-bit output of stream(seed, i, j + 1), made once per (seed, centre, position)"""
    memo = _CACHE.setdefault(("draws", seed, i), {})
    return [memo[j] if j in memo else memo.setdefault(j, int(stream(seed, i, j + 1, 1)[0])) for j in js]


def typed_sample(row_ptr, col, edge_type, centers, fanouts, seed=0, draw=draws, live_counts=None):
    """-> offsets int32 [n + 1], ids (col's dtype), center local id int32, edge id int64, edge type int32. live_counts: a list
    that receives E_ir of every centre as a list over r"""
    n_nodes, n_edges, R = len(row_ptr) - 1, len(col), len(fanouts)
    assert len(edge_type) == n_edges and 1 <= R <= 64 and min(fanouts) >= 0 and 1 <= sum(fanouts) <= 64
    offsets, lid, egid = [0], [], []
    for k, u in enumerate(int(x) for x in centers):
        per_relation = [[] for _ in range(R)]
        s = 0
        if 0 <= u < n_nodes and row_valid(int(row_ptr[u]), int(row_ptr[u + 1]), n_edges):
            s = int(row_ptr[u])
            for j, ty in enumerate(edge_type[s:int(row_ptr[u + 1])].tolist()):
                if 0 <= ty < R and fanouts[ty] > 0:
                    per_relation[ty].append(j)
        if live_counts is not None:
            live_counts.append([len(js) for js in per_relation])
        kept = []
        for js, f in zip(per_relation, fanouts):
            kept += select(js, draw(seed, k, js), f) if len(js) > f else js
        kept.sort()
        lid += [k] * len(kept)
        egid += [s + j for j in kept]
        offsets.append(len(egid))
    egid = np.array(egid, dtype=np.int64)
    return (np.array(offsets, dtype=np.int32), np.asarray(col)[egid], np.array(lid, dtype=np.int32), egid,
            np.asarray(edge_type)[egid].astype(np.int32))


def typed_ladder():
    """-> row_ptr, col, edge_type int32, starts int64 [512] of _walk_ref.ladder() (read-only, shared); types random in 0 .. 3 but
    node 7 (5000 neighbours) skewed, nine in ten of relation 0; node 8 (1024) of relation 2 alone; node 9 (1025) with -1 at every
    7th and 4 (= R) at every 11th entry; node 11 (64) with exactly 8 entries of relation 1 and four of relation 3."""
    if "ladder" not in _CACHE:
        row_ptr, col, _, starts = ladder()
        ty = np.random.default_rng(79).integers(0, LADDER_R, col.shape[0]).astype(np.int32)
        k = np.arange(5000)
        ty[row_ptr[7]:row_ptr[8]] = np.where(k % 10 != 9, 0, 1 + (k // 10) % 3)
        ty[row_ptr[8]:row_ptr[9]] = 2
        ty[row_ptr[9]:row_ptr[10]:7] = -1
        ty[row_ptr[9] + 3:row_ptr[10]:11] = LADDER_R
        k = np.arange(64)
        ty[row_ptr[11]:row_ptr[12]] = np.where(k % 8 == 5, 1, np.where(k % 20 == 0, 3, (k % 2) * 2))
        ty.setflags(write=False)
        _CACHE["ladder"] = (row_ptr, col, ty, starts)
    return _CACHE["ladder"]


def ladder_sample(fanouts=LADDER_FANOUTS):
    """the reference outputs on the ladder's 512 centres, with E_ir [512, R] as a sixth entry"""
    key = ("sample", tuple(fanouts))
    if key not in _CACHE:
        row_ptr, col, ty, starts = typed_ladder()
        counts = []
        out = typed_sample(row_ptr, col, ty, starts, list(fanouts), LADDER_SEED, live_counts=counts)
        _CACHE[key] = out + (np.array(counts, dtype=np.int64),)
    return _CACHE[key]


def assert_ladder_measures():
    """what the typed ladder must exercise at its fan-outs, on the REFERENCE, so that a later change cannot empty a case; and
    the point of the op: on the skewed row every relation with at least 8 edges gets its 8 samples"""
    offsets, _, _, _, types, live = ladder_sample()
    f = np.array(LADDER_FANOUTS)
    got = {"no_selection": int((live <= f).all(axis=1).sum()), "selection": int((live > f).any(axis=1).sum()),
           "exactly_f": int((live == f).any(axis=1).sum()), "one_relation_only": int(((live > 0).sum(axis=1) == 1).sum()),
           "mixed": int(((live > f).any(axis=1) & (live < f).any(axis=1) & (live > 0).all(axis=1)).sum())}
    assert min(got.values()) >= 1, got
    assert live[7].tolist() == [4500, 167, 167, 166] and live[11].tolist() == [28, 8, 24, 4] and live[8].tolist() == [0, 0, 1024, 0]
    assert np.bincount(types[offsets[7]:offsets[8]], minlength=LADDER_R).tolist() == [8, 8, 8, 8]
    return got
