"""The device row cache's replacement policy against the plain-Python model of tests/_row_cache_model.py: after every batch
the hits, the occupied lines, the slots and the lookups EQUAL the model's, at the end of a stream the resident set does, row by
row. The existing cache tests show that the cache is transparent; these show that it keeps the rows kernels/cache.hip says it
keeps (one wave per set walks its rows in order, so the device is reproducible and the model can predict it exactly).
tests/test_row_cache_model.py shows that each of these streams would expose a kernel that picks the wrong victim, admits on a
tie, breaks ties by the wrong lane or counts after replacing. Every gather is also compared bit for bit with the closed-form
table, -1 at every 17th position."""
import ctypes as C

import numpy as np
import pytest

import oracle
import _row_cache_model as M

pytestmark = pytest.mark.gpu

DIM = 8


def _info(emb):
    from wholegraph_amd import binding as wmb
    v = [C.c_int64() for _ in range(5)]
    wmb.check(wmb.lib().wholememory_ext_embedding_cache_info(emb.wmb_embedding, *[C.byref(x) for x in v]))
    return dict(zip(("slots", "occupied", "dirty", "hits", "lookups"), [x.value for x in v]))


# how each stream's table and cache are made: (table memory type, table location, cache: "own" = the embedding's communicator
# (every rank caches its shard) | "local" = another communicator (a local read-only cache of the whole table), access)
SETUP = {
    "1501-zipf": ("chunked", "cpu", "own", "readonly"),
    "1501-uniform": ("chunked", "cpu", "own", "readonly"),
    "1501-shifting": ("chunked", "cpu", "own", "readonly"),
    "2309-zipf": ("chunked", "cuda", "own", "readonly"),
    "130-uniform": ("distributed", "cpu", "own", "readonly"),
    "40-uniform": ("chunked", "cuda", "local", "readonly"),
    "65-uniform": ("chunked", "cpu", "own", "readwrite"),
}
CASES = [(name, idt) for name in ("1501-zipf", "1501-uniform", "1501-shifting", "2309-zipf") for idt in (np.int64, np.int32)] + \
        [("130-uniform", np.int64), ("40-uniform", np.int64), ("65-uniform", np.int32)]


class _Device:
    """an embedding with a row cache over the closed-form table, and the model next to it"""

    def __init__(self, comm, name, idt):
        import torch
        import wholegraph_amd.torch as wgth
        self.torch, self.wgth, self.idt = torch, wgth, idt
        self.rows, ratio, self.batches = M.policy_stream(name)
        mt, loc, whose, access = SETUP[name]
        cache_comm = comm if whose == "own" else wgth.create_group_communicator(1)
        self.policy = wgth.create_wholememory_cache_policy(cache_comm, memory_type=mt if whose == "own" else "continuous",
                                                           memory_location="cuda", access_type=access, ratio=ratio)
        self.emb = wgth.create_embedding(comm, mt, loc, torch.float32, [self.rows, DIM], cache_policy=self.policy)
        self.full = oracle.fill_closed_form(np.float32, 0, self.rows, DIM)
        local, _ = self.emb.get_embedding_tensor().get_local_tensor(host_view=loc == "cpu")
        local.copy_(torch.from_numpy(self.full))
        torch.cuda.synchronize()
        self.model = M.RowCacheModel(self.rows, ratio, owner_side=whose == "own")
        self.check_state()

    def check_state(self):
        info, m = _info(self.emb), self.model
        assert info["slots"] == 64 * m.n_sets
        assert (info["occupied"], info["dirty"], info["hits"], info["lookups"]) == (m.occupied, 0, m.hits, m.lookups), \
            (info, m.occupied, m.hits, m.lookups)

    def gather(self, ids, adjust, what):
        """one gather on the device and in the model; returns the hits"""
        torch = self.torch
        ids = np.asarray(ids).astype(self.idt)
        self.emb.set_adjust_cache(adjust)
        before = _info(self.emb)
        out = torch.full((len(ids), DIM), -7.0, device="cuda")
        self.emb.gather(torch.from_numpy(ids).cuda(), out=out)
        torch.cuda.synchronize()
        want = np.full((len(ids), DIM), -7.0, np.float32)
        want[ids >= 0] = self.full[ids[ids >= 0]]
        assert out.cpu().numpy().tobytes() == want.tobytes(), "%s: rows differ from the table" % what
        after = _info(self.emb)
        lookups0 = self.model.lookups
        hits = self.model.gather(ids, adjust)
        assert after["hits"] - before["hits"] == hits, "%s: hits %d, the model's %d" % (what, after["hits"] - before["hits"], hits)
        assert after["occupied"] == self.model.occupied, "%s: occupied %d, the model's %d" % (what, after["occupied"], self.model.occupied)
        assert after["slots"] == 64 * self.model.n_sets and after["dirty"] == 0
        assert after["lookups"] - before["lookups"] == self.model.lookups - lookups0, what
        return hits

    def resident(self):
        """the resident rows, found by asking for every row on its own with adjustment off: a hit or none"""
        torch = self.torch
        self.emb.set_adjust_cache(False)
        all_ids = torch.arange(self.rows, dtype=torch.int64 if self.idt == np.int64 else torch.int32, device="cuda")
        found, hits = [], _info(self.emb)["hits"]
        for r in range(self.rows):
            got = self.emb.gather(all_ids[r:r + 1])
            now = _info(self.emb)["hits"]
            assert now - hits in (0, 1)
            if now != hits:
                found.append(r)
            hits = now
            if r % 97 == 0:
                assert got.cpu().numpy().tobytes() == self.full[r:r + 1].tobytes()
        self.model.lookup(np.arange(self.rows))
        return np.array(found, dtype=np.int64)

    def close(self):
        self.wgth.destroy_embedding(self.emb)
        self.wgth.destroy_wholememory_cache_policy(self.policy)


@pytest.mark.parametrize("name,idt", CASES, ids=["%s-%s" % (n, np.dtype(t).name) for n, t in CASES])
def test_device_follows_the_policy_model(gpu_env, name, idt):
    d = _Device(gpu_env, name, idt)
    m = d.model
    assert (m.n_sets, m.set_cover) == {"1501": (3, 501), "2309": (10, 231), "130-": (2, 65), "40-u": (1, 40), "65-u": (2, 33)}[name[:4]]
    first_pass = []
    for b, ids in enumerate(d.batches):
        first_pass.append(d.gather(ids, True, "batch %d" % b))
        if b == 4:
            # a batch with adjustment off: a lookup and nothing else — residency stays (occupied, and the resident set at the
            # end), and so do the counters: the batches that follow keep agreeing with the model, which counted nothing here
            rows_before = m.resident().copy()
            d.gather(d.batches[0][::-1], False, "unadjusted batch")
            assert np.array_equal(m.resident(), rows_before)
    assert np.array_equal(d.resident(), m.resident()), "resident set differs from the model's"
    d.check_state()
    # drop: an empty cache AND cleared counters — the same stream then replays the same hits (with the old counters the
    # first batch would meet rows that are admitted by counters it never earned)
    d.emb.drop_all_cache()
    m.drop()
    d.check_state()
    assert m.occupied == 0
    second_pass = [d.gather(ids, True, "replayed batch %d" % b) for b, ids in enumerate(d.batches)]
    assert second_pass == first_pass, (first_pass, second_pass)
    d.check_state()
    d.close()
