"""The device row cache's replacement policy in plain Python and numpy: what kernels/cache.hip states in its header, written
down a second time without looking at how the kernels do it. Shared by tests/test_row_cache_model.py (hand-worked cases, the
mutants), tests/test_row_cache_policy_gpu.py and tests/test_row_cache_training_gpu.py (the device against this model). It does
not import the library.

Sizing (embedding_cache.cpp: create_row_cache): slots = int(cover_rows * ratio) clamped to [64, cover_rows + 63], n_sets =
ceil(slots / 64), set_cover = ceil(cover_rows / n_sets); set s covers the rows [s * set_cover, (s + 1) * set_cover), cut at
cover_rows — the last set may be shorter. With ratios that are powers of two the product is exact in float and in double.

Policy (kernels/cache.hip, header and cache_update_kernel):
 * every covered row has an exact counter; a batch first adds each row's multiplicity to it (cache_count_kernel). Ids outside
   [0, cover_rows) — the negative "skip" ids among them — count nowhere;
 * then every set walks ITS unique batch rows in ascending order. A resident row is passed over. For a missing row the victim is
   the slot with the smallest (counter of its resident row, lane); an empty slot counts as -1, so empty slots go first, in lane
   order. The row is admitted only if its counter is strictly greater than the victim's; the victim's row leaves;
 * a modified line that leaves is written back to the table first; the refilled line is clean;
 * write-back clears the dirty bits; drop also empties every slot and clears every counter.
A row that leaves in a batch and is met later in the same batch stays out: it left as the set's minimum, so what is resident now
has at least its counter.

Where the library calls what (the order matters: an update BEFORE the lookup makes a batch hit on the rows it brought in):
 * ops.cpp gather_cached / gather_distributed_rows: row_cache_update first — only with adjust_cache —, then row_cache_gather
   (the lookup, which counts hits and lookups)                                                               -> gather()
 * embedding.cpp owner_apply: row_cache_update first — only with adjust_cache —, then the step kernels, which mark the lines of
   resident rows modified (optim.hip: cache_dirty)                                                            -> apply_gradients()
 * embedding.cpp create_states -> embedding_cache.cpp row_cache_attach_states: an optimizer WITH per-element states (every one
   but SGD) drops the cache when it is attached                                                               -> attach_states()
 * wholememory_embedding_writeback_cache / _drop_all_cache                                                    -> writeback() / drop()
"""
import numpy as np

SET_SLOTS = 64


def sizing(cover_rows, ratio):
    """(n_sets, set_cover) of a cache over cover_rows rows"""
    if cover_rows <= 0:
        return 0, 0
    slots = int(cover_rows * ratio)
    slots = min(cover_rows + SET_SLOTS - 1, max(slots, SET_SLOTS))
    n_sets = (slots + SET_SLOTS - 1) // SET_SLOTS
    return n_sets, (cover_rows + n_sets - 1) // n_sets


class RowCacheModel:
    # the three decisions of the policy; tests/test_row_cache_model.py overrides them one at a time to build its mutants
    count_first = True

    def pick_victim(self, counters):
        """lane of the victim among the 64 (counter, lane) of a set; counters: int64[64], -1 = empty slot"""
        return int(np.argmin(counters))     # the first of the minima: the lowest lane

    def admits(self, candidate_counter, victim_counter):
        return candidate_counter > victim_counter

    def __init__(self, cover_rows, ratio, owner_side=True):
        """owner_side: the cache of a rank's own shard (cache communicator = the embedding's) — it sees the ids that reach the
        owner, and an id that addresses no row reaches none. False: a local cache of the whole table, which sees every id."""
        self.owner_side = owner_side
        self.cover_rows = int(cover_rows)
        self.n_sets, self.set_cover = sizing(self.cover_rows, ratio)
        self.slots = self.n_sets * SET_SLOTS
        self.count = np.zeros(self.cover_rows, np.int64)
        self.slot_of = np.full(self.cover_rows, -1, np.int64)
        self.row_of = np.full(self.slots, -1, np.int64)
        self.dirty = np.zeros(self.slots, bool)
        self.hits = 0
        self.lookups = 0
        # events, summed over all updates
        self.evictions = 0            # a resident row left
        self.equal_decisions = 0      # a candidate met a victim with exactly its counter (and stayed out)
        self.in_batch_evictions = 0   # the row that left occurs in the same batch
        self.met_again = 0            # ... and behind the candidate: the walk meets it again, missing now
        self.written_back = []        # rows that left while modified, in order

    def set_rows(self, s):
        lo = s * self.set_cover
        return lo, min(self.cover_rows, lo + self.set_cover)

    def _valid(self, ids):
        ids = np.asarray(ids).astype(np.int64)
        return ids[(ids >= 0) & (ids < self.cover_rows)]

    # ---- the cache's own operations
    def update(self, ids):
        """one batch: counters, then replacement. Returns the rows that were written back (left while modified)."""
        uniq, mult = np.unique(self._valid(ids), return_counts=True)
        if self.count_first:
            self.count[uniq] += mult
        in_batch = set(uniq.tolist())
        out = []
        for s in np.unique(uniq // self.set_cover).tolist() if len(uniq) else []:
            lo, hi = self.set_rows(s)
            base = s * SET_SLOTS
            lanes = self.row_of[base:base + SET_SLOTS]        # a view: residents by lane
            counters = np.where(lanes >= 0, self.count[np.maximum(lanes, 0)], -1)
            for r in uniq[(uniq >= lo) & (uniq < hi)].tolist():
                if self.slot_of[r] >= 0:
                    continue
                cand = int(self.count[r])
                lane = self.pick_victim(counters)
                if cand == counters[lane]:
                    self.equal_decisions += 1
                if not self.admits(cand, int(counters[lane])):
                    continue
                old = int(lanes[lane])
                if old >= 0:
                    self.evictions += 1
                    if old in in_batch:
                        self.in_batch_evictions += 1
                        self.met_again += old > r
                    if self.dirty[base + lane]:
                        out.append(old)
                    self.slot_of[old] = -1
                self.slot_of[r] = base + lane
                lanes[lane] = r
                counters[lane] = cand
                self.dirty[base + lane] = False
        if not self.count_first:
            self.count[uniq] += mult
        self.written_back += out
        return out

    def lookup(self, ids):
        """hits of a batch. Lookups: the ids the cache is asked for — ops.cpp gather_distributed_rows hands the owner's cache
        the ids that were bucketed to this owner (ids that address no row, the negative "skip" ids among them, are bucketed to
        nobody), gather_cached hands a local cache the caller's batch as it stands"""
        valid = self._valid(ids)
        h = int((self.slot_of[valid] >= 0).sum())
        self.hits += h
        self.lookups += len(valid) if self.owner_side else len(ids)
        return h

    def train(self, ids):
        slots = self.slot_of[self._valid(ids)]
        self.dirty[slots[slots >= 0]] = True

    def writeback(self):
        self.dirty[:] = False

    def drop(self):
        self.slot_of[:] = -1
        self.row_of[:] = -1
        self.dirty[:] = False
        self.count[:] = 0

    # ---- the library's calls
    def gather(self, ids, adjust=True):
        if adjust:
            self.update(ids)
        return self.lookup(ids)

    def apply_gradients(self, ids, adjust=True):
        out = self.update(ids) if adjust else []
        self.train(ids)
        return out

    def attach_states(self):
        self.drop()

    # ---- what the tests read
    @property
    def occupied(self):
        return int((self.row_of >= 0).sum())

    @property
    def n_dirty(self):
        return int(self.dirty.sum())

    def resident(self):
        """sorted resident rows"""
        return np.sort(self.row_of[self.row_of >= 0])

    def resident_dirty(self):
        return np.sort(self.row_of[(self.row_of >= 0) & self.dirty])


# ---- id streams of the policy tests: a list of batches each, -1 at every 17th position ------------------------------------
def _zipf(rng, n, n_rows):
    k = rng.zipf(1.2, n).astype(np.uint64)
    return ((k * np.uint64(2654435761)) % np.uint64(n_rows)).astype(np.int64)


def stream(kind, n_rows, batches=10, per_batch=400, seed=5):
    """kind: "zipf" | "uniform" | "shifting" (Zipf whose ids move on by 37 rows per batch: yesterday's hot rows cool down)"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(batches):
        if kind == "uniform":
            ids = rng.integers(0, n_rows, per_batch).astype(np.int64)
        else:
            ids = _zipf(rng, per_batch, n_rows)
            if kind == "shifting":
                ids = (ids + 37 * b) % n_rows
        ids[::17] = -1
        ids.setflags(write=False)
        out.append(ids)
    return out


# (name, rows, ratio, stream kind, ids per batch, seed): every stream the device test replays, 10 batches each. The first five
# reach replacement decisions (a set covers more than 64 rows); in the last two every covered row has a slot of its own, so
# nothing is ever evicted — they pin the sizing edges (one set of fewer than 64 rows; two sets of 33 and 32 rows).
# Batch sizes and seeds are chosen so that tests/test_row_cache_model.py's conditions hold (events reached, mutants told apart).
POLICY_STREAMS = [
    ("1501-zipf", 1501, 0.125, "zipf", 600, 1),
    ("1501-uniform", 1501, 0.125, "uniform", 400, 2),
    ("1501-shifting", 1501, 0.125, "shifting", 600, 1),
    ("2309-zipf", 2309, 0.25, "zipf", 600, 1),
    ("130-uniform", 130, 0.5, "uniform", 400, 1),
    ("40-uniform", 40, 0.5, "uniform", 400, 1),
    ("65-uniform", 65, 1.0, "uniform", 400, 1),
]
REPLACING_STREAMS = [s[0] for s in POLICY_STREAMS[:5]]


def policy_stream(name):
    """(rows, ratio, batches) of a named stream"""
    for nm, rows, ratio, kind, per_batch, seed in POLICY_STREAMS:
        if nm == name:
            return rows, ratio, stream(kind, rows, 10, per_batch, seed)
    raise KeyError(name)
