"""The node-induced subgraph as include/wholememory/wholegraph_amd_ext.h section 2q defines it, restated in plain Python: the
reference of tests/test_isub_gpu.py and tests/test_saint_gpu.py (against the kernels of csrc/kernels/isub.hip). Two forms: a
loop that follows the definition sentence by sentence, and a vectorised numpy form for the large case; they are asserted
equal on the ladder of tests/_walk_ref.py (ladder_subgraph). Also the reference outputs on the ladder, computed once and shared."""
import numpy as np

_CACHE = {}


def row_valid(s, e, n_edges):
    """the damaged-graph rule of sections 2m - 2o: bounds that are a row"""
    return 0 <= s <= e <= n_edges and e - s < (1 << 31)


def first_positions(nodes, n_nodes):
    """{member v: first(v)}: the lowest i with nodes[i] == v, for the v in [0, n_nodes)"""
    first = {}
    for i, v in enumerate(int(x) for x in nodes):
        if 0 <= v < n_nodes and v not in first:
            first[v] = i
    return first


def induced_subgraph(row_ptr, col, nodes):
    """the loop form -> offsets int32 [n + 1], col int32 [m], edge ids int64 [m]"""
    n_nodes, n_edges = len(row_ptr) - 1, len(col)
    first = first_positions(nodes, n_nodes)
    offsets, out_col, out_eid = [0], [], []
    for u in (int(x) for x in nodes):
        if 0 <= u < n_nodes:
            s, e = int(row_ptr[u]), int(row_ptr[u + 1])
            if row_valid(s, e, n_edges):
                for pos in range(s, e):
                    c = int(col[pos])
                    if c in first:          # (compared, never used as an index)
                        out_col.append(first[c])
                        out_eid.append(pos)
        offsets.append(len(out_col))
    assert offsets[-1] < 1 << 31
    return np.array(offsets, dtype=np.int32), np.array(out_col, dtype=np.int32), np.array(out_eid, dtype=np.int64)


def induced_subgraph_vectorised(row_ptr, col, nodes):
    """the same in numpy, for many rows"""
    row_ptr, col, nodes = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(nodes, dtype=np.int64)
    n_nodes, n_edges, n = row_ptr.shape[0] - 1, col.shape[0], nodes.shape[0]
    inside = (nodes >= 0) & (nodes < n_nodes)
    first_of = np.full(n_nodes + 1, -1, dtype=np.int64)           # node -> first position; slot n_nodes stays -1
    idx = np.nonzero(inside)[0]
    first_of[nodes[idx[::-1]]] = idx[::-1]                          # (the lowest position is written last)
    u = np.where(inside, nodes, 0)
    s, e = row_ptr[u], row_ptr[np.minimum(u + 1, n_nodes)]
    ok = inside & (s >= 0) & (s <= e) & (e <= n_edges) & (e - s < (1 << 31))
    length = np.where(ok, e - s, 0)
    start = np.concatenate([[0], np.cumsum(length)])
    row_of = np.repeat(np.arange(n), length)
    pos = np.arange(start[-1]) - start[row_of] + s[row_of]
    c = col[pos]
    local = first_of[np.where((c >= 0) & (c < n_nodes), c, n_nodes)]
    keep = local >= 0
    counts = np.bincount(row_of[keep], minlength=n)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    assert offsets[-1] < 1 << 31
    return offsets.astype(np.int32), local[keep].astype(np.int32), pos[keep].astype(np.int64)


def ladder_subgraph():
    """the subgraph the ladder's 512 starts induce (loop form, asserted equal to the vectorised one) -> offsets, col, edge ids"""
    if "ladder" not in _CACHE:
        from _walk_ref import ladder
        row_ptr, col, _, starts = ladder()
        want = induced_subgraph(row_ptr, col, starts)
        fast = induced_subgraph_vectorised(row_ptr, col, starts)
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(want, fast)), "the two forms of the reference differ"
        for a in want:
            a.setflags(write=False)
        _CACHE["ladder"] = want
    return _CACHE["ladder"]


def ladder_measures():
    """what the ladder must exercise, measured on the REFERENCE"""
    from _walk_ref import LADDER_NODES, ladder
    row_ptr, _, _, starts = ladder()
    offsets = ladder_subgraph()[0].astype(np.int64)
    length = np.diff(offsets)
    inside = (starts >= 0) & (starts < LADDER_NODES)
    degree = np.where(inside, row_ptr[np.where(inside, starts, 0) + 1] - row_ptr[np.where(inside, starts, 0)], 0)
    first = first_positions(starts, LADDER_NODES)
    duplicates = sum(1 for i, v in enumerate(int(x) for x in starts) if v in first and first[v] != i)
    return {"m": int(offsets[-1]), "row_of_7": int(length[first[7]]), "empty_rows": int((length == 0).sum()),
            "duplicates": duplicates, "refused": int((~inside).sum()),
            "partial_rows": int(((length > 0) & (length < degree)).sum()),
            "rows": {v: int(length[first[v]]) for v in (8, 9, 10, 11, 14)}}
