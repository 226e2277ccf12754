"""PinSAGE importance neighbourhoods as section 2s of include/wholememory/wholegraph_amd_ext.h defines them, in plain Python:
the reference of tests/test_rwr_gpu.py, over the generator (stream) and the graphs (ladder, star) of tests/_walk_ref.py."""
import numpy as np

from _walk_ref import stream


def rwr_top(row_ptr, col, seeds, R, L, restart_prob, T, seed):
    """-> nodes int64 [n, T], counts int32 [n, T], and what the walks met (a dict of counters)"""
    n_nodes, n_edges, n = row_ptr.shape[0] - 1, col.shape[0], len(seeds)
    thr = int(restart_prob * 4294967296.0)
    nodes, counts = np.full((n, T), -1, dtype=np.int64), np.zeros((n, T), dtype=np.int32)
    met = dict(trunc=0, tie_at_cut=0, dead=0, restarts=0, short=0, maxdistinct=0)
    for i, s in enumerate(int(x) for x in seeds):
        if not 0 <= s < n_nodes:
            continue
        visits = {}
        for r in range(R):
            draws, v = stream(seed, i * R + r, 0, 2 * L), s
            for t in range(L):
                a, b = int(draws[2 * t]), int(draws[2 * t + 1])
                if a < thr:
                    met["restarts"] += 1
                    v = s
                    continue
                lo, hi = int(row_ptr[v]), int(row_ptr[v + 1])
                c = -1
                if lo >= 0 and hi > lo and hi <= n_edges and hi - lo < 1 << 31:
                    c = int(col[lo + ((b * (hi - lo)) >> 32)])
                if not 0 <= c < n_nodes:
                    met["dead"] += 1
                    v = s
                    continue
                v = c
                if c != s:
                    visits[c] = visits.get(c, 0) + 1
        ranked = sorted(visits.items(), key=lambda kv: (-kv[1], kv[0]))
        met["trunc"] += len(ranked) > T
        met["tie_at_cut"] += len(ranked) > T and ranked[T - 1][1] == ranked[T][1]
        met["short"] += len(ranked) < T
        met["maxdistinct"] = max(met["maxdistinct"], len(ranked))
        for k, (node, count) in enumerate(ranked[:T]):
            nodes[i, k], counts[i, k] = node, count
    return nodes, counts, met
