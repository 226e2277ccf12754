"""Negative sampling as include/wholememory/wholegraph_amd_ext.h section 2o defines it, restated in plain Python: the reference
of tests/test_neg_streams.py (against the host/device header csrc/neg_sample.hpp) and of tests/test_neg_gpu.py (against the
kernel). The streams are tests/_walk_ref.py's; the 128-bit products are Python integers and "c occurs in the row of u" is asked
of a Python set per row. Also the graphs of the GPU tests — the ladder, its row-sorted copy, the dozen — whose reference
outputs are computed once and shared."""
import numpy as np

import _walk_ref as wref

_DRAWS = {}
_CACHE = {}


def draws64(seed, j, tries):
    """the first `tries` 64-bit draws of stream(seed, j, 0) as Python integers: two 32-bit outputs each, low word first"""
    got = _DRAWS.get((seed, j))
    if got is None or len(got) < tries:
        d = wref.stream(seed, j, 0, 2 * max(tries, 16))
        got = [int(d[2 * a]) | (int(d[2 * a + 1]) << 32) for a in range(d.shape[0] // 2)]
        _DRAWS[(seed, j)] = got
    return got


def negative_samples(row_ptr, col, src, num_negatives, mode, exclude, max_tries, seed, first_source=0, out_of_range=None,
                     numbers=None):
    """-> int64 [n, K]. mode 0 uniform, 1 by degree; exclude bit 0 the neighbours, bit 1 the source. first_source: the number of
    src[0] in the batch it was cut from (source i of the result uses the streams of source first_source + i), or numbers: the
    number of every source in that batch. out_of_range: a dict that counts, per value, the candidates rejected for lying
    outside [0, n_nodes)."""
    row_ptr, col = np.asarray(row_ptr), np.asarray(col)
    n_nodes, n_edges, K = row_ptr.shape[0] - 1, col.shape[0], int(num_negatives)
    out = np.full((len(src), K), -1, dtype=np.int64)
    nobody = frozenset()
    rows = {}
    for i, u in enumerate(int(x) for x in src):
        if not 0 <= u < n_nodes:
            continue
        near = nobody
        if exclude & 1:
            s, e = int(row_ptr[u]), int(row_ptr[u + 1])
            if 0 <= s <= e <= n_edges and e - s < 1 << 31:      # (a source whose bounds are not a row excludes no edge)
                if u not in rows:
                    rows[u] = frozenset(int(x) for x in col[s:e])
                near = rows[u]
        for k in range(K):
            r = draws64(seed, (first_source + i if numbers is None else int(numbers[i])) * K + k, max_tries)
            for a in range(max_tries):
                if mode == 0:
                    c = (r[a] * n_nodes) >> 64
                elif n_edges == 0:
                    continue
                else:
                    c = int(col[(r[a] * n_edges) >> 64])
                if not 0 <= c < n_nodes:
                    if out_of_range is not None:
                        out_of_range[c] = out_of_range.get(c, 0) + 1
                    continue
                if (exclude & 2 and c == u) or c in near:
                    continue
                out[i, k] = c
                break
    return out


def assert_outputs_allowed(out, row_ptr, col, src, exclude, what=""):
    """every output is -1 or a node; none is a neighbour of its source (exclude & 1) or the source (exclude & 2)"""
    out, col = np.asarray(out, dtype=np.int64), np.asarray(col)
    n_nodes = row_ptr.shape[0] - 1
    assert ((out == -1) | ((out >= 0) & (out < n_nodes))).all(), what
    for i, u in enumerate(int(x) for x in src):
        if not 0 <= u < n_nodes:
            assert (out[i] == -1).all(), (what, i)
            continue
        if exclude & 2:
            assert not (out[i] == u).any(), (what, i)
        if exclude & 1:
            assert not np.isin(out[i][out[i] >= 0], col[int(row_ptr[u]):int(row_ptr[u + 1])]).any(), (what, i)


# ------------------------------------------------------------------------------------------------ the ladder
SEED = 2718
KS, TRIES = (1, 5, 33), (1, 8)


def ladder(in_order=False):
    """_walk_ref.ladder() (2000 nodes, one row of 5000, rows of 63 / 64 / 65 / 1024 / 1025, an empty row), or its copy with
    every row ascending -> row_ptr, col, sources int64 [512] (read-only, shared): the starts of the walks, which hold the three
    refused ids and nodes 7 .. 15"""
    key = ("ladder", bool(in_order))
    if key not in _CACHE:
        row_ptr, col, _, starts = wref.ladder()
        if in_order:
            col = np.array(col)
            for v in range(row_ptr.shape[0] - 1):
                col[row_ptr[v]:row_ptr[v + 1]].sort()
            col.setflags(write=False)
        assert set(range(7, 16)) <= set(starts.tolist()) and {-1, wref.LADDER_NODES, wref.LADDER_NODES + 5} <= set(starts.tolist())
        _CACHE[key] = (row_ptr, col, starts)
    return _CACHE[key]


def ladder_negatives(in_order, num_negatives, mode, exclude, max_tries):
    key = ("negatives", bool(in_order), num_negatives, mode, exclude, max_tries)
    if key not in _CACHE:
        row_ptr, col, src = ladder(in_order)
        # (membership does not depend on the order of a row: the sorted copy has the outputs of the ladder in mode 0)
        shared = ("negatives", False, num_negatives, mode, exclude, max_tries)
        if in_order and mode == 0 and shared in _CACHE:
            _CACHE[key] = _CACHE[shared]
        else:
            _CACHE[key] = negative_samples(row_ptr, col, src, num_negatives, mode, exclude, max_tries, SEED)
            _CACHE[key].setflags(write=False)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the dozen
DOZEN_SOURCES, DOZEN_K, DOZEN_SEED = 3000, 8, 2024


def dozen():
    """12 nodes. Node 0 has the row [1, 2, 3, 4, 5]; rows 1 .. 11 hold 3 .. 7 entries each, drawn with default_rng(11) so that
    node j is pointed at in proportion to j + 1 (skewed in-degrees), every row ascending. With exclude = 3 the negatives of
    node 0 are 6 .. 11. -> row_ptr, col"""
    if "dozen" not in _CACHE:
        rng = np.random.default_rng(11)
        share = np.arange(1, 13, dtype=np.float64)
        share /= share.sum()
        rows = [[1, 2, 3, 4, 5]]
        for _ in range(1, 12):
            rows.append(sorted(int(x) for x in rng.choice(12, size=int(rng.integers(3, 8)), p=share)))
        row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        col = np.array([x for r in rows for x in r], dtype=np.int64)
        assert all((col == j).sum() > 0 for j in range(6, 12))
        _CACHE["dozen"] = (row_ptr, col)
    return _CACHE["dozen"]


def dozen_statistic(out, mode):
    """-> (share of -1, chi-square over 5 degrees of freedom of the outputs that are not -1 against: mode 0, uniform over
    6 .. 11; mode 1, the counts of 6 .. 11 in col_ind, normalised)"""
    out = np.asarray(out, dtype=np.int64)
    assert out.shape == (DOZEN_SOURCES, DOZEN_K)
    drawn = out[out >= 0]
    assert drawn.min() >= 6 and drawn.max() <= 11 and (out[out < 0] == -1).all()
    col = dozen()[1]
    expect = np.ones(6) if mode == 0 else np.array([(col == j).sum() for j in range(6, 12)], dtype=np.float64)
    expect = expect / expect.sum() * drawn.shape[0]
    counts = np.bincount(drawn - 6, minlength=6)
    return float((out < 0).mean()), float(((counts - expect) ** 2 / expect).sum())


# (mode, max_tries) -> (outputs that are -1 of 24 000, chi-square). The seed and the graph were fixed before the values were
# computed (tests/test_neg_streams.py computes them with the host program; the kernel draws the same samples, so
# tests/test_neg_gpu.py asks for the same values; DESIGN.md 3.19 states them)
DOZEN_VALUES = {(0, 16): (1, 6.9204966873619735), (1, 16): (0, 3.682261904761905), (0, 4): (1486, 7.444256906813539)}
