"""Training through a read-write device row cache on the shapes whose cached step kernels no other test launches: lines of
more than 1024 bytes (the second and third trip of the cache's row copy, for rows and for the companion state lines), the cached
8-byte and 4-byte short kernels, RMSProp and the tree fold through a cache, and every cached 16-bit instantiation.

A HOST table (chunked) with a DEVICE cache of a quarter of its rows, 4001 rows, 6000 ids per step, every third id one hot id
(a run of 2000 rows: the long-run side), the rest half Zipf, half uniform. The reference is the CPU oracle with a padded stride —
never the uncached library — and tests/_row_cache_model.py says which rows are resident and modified. Four steps:
 1 adjustment on;
 2 drop_all_cache(), then a step with adjustment off: every row misses, the cached kernels still run;
 3 a gather in training mode, then a step, adjustment on;
 4 other ids, adjustment on: lines modified by step 3 leave the cache and are written back by the replacement itself.
After each step a probe gather (adjustment off) equals the oracle bit for bit, dirty and occupied equal the model's, and every
raw host row — and optimizer state row — that the model does not hold resident-and-modified equals the oracle's: lines that left
were written back, rows that missed were stepped in the table. At the end write-back, dirty == 0, and the whole raw table and
every state table equal the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle
import _row_cache_model as M

pytestmark = pytest.mark.gpu

N_ROWS, N_IDS, RATIO, HOT = 4001, 6000, 0.25, 2007


def _info(emb):
    from wholegraph_amd import binding as wmb
    v = [C.c_int64() for _ in range(5)]
    wmb.check(wmb.lib().wholememory_ext_embedding_cache_info(emb.wmb_embedding, *[C.byref(x) for x in v]))
    return dict(zip(("slots", "occupied", "dirty", "hits", "lookups"), [x.value for x in v]))


def _ids(rng, shift, idt):
    k = rng.zipf(1.2, N_IDS).astype(np.uint64)
    zipf = ((k * np.uint64(2654435761)) % np.uint64(N_ROWS)).astype(np.int64)
    ids = np.where(rng.random(N_IDS) < 0.5, zipf, rng.integers(0, N_ROWS, N_IDS))
    ids = (ids + shift) % N_ROWS
    ids[::3] = HOT
    return ids.astype(idt)


def _normal_grads(rng, ids, dim):
    return rng.standard_normal((len(ids), dim)).astype(np.float32)


def _integer_grads(rng, ids, dim):
    """as in test_tree_fold_exact_on_integer_gradients: every partial sum is an integer below 2^24, exact in fp32 in any order"""
    return rng.integers(-3, 4, (len(ids), dim)).astype(np.float32)


def _sparse_integer_grads(rng, ids, dim):
    """-1 / 0 / +1, so sparse on the ids with many copies that no element of a row collects more than 60 non-zero terms in a
    step: every partial sum, in any grouping, and every result (|start| <= 8, four steps: <= 248) is an integer of at most
    8 significant bits — exact in bfloat16 and float16 as well as in fp32"""
    mult = np.bincount(ids, minlength=N_ROWS)[ids]
    g = rng.integers(-1, 2, (len(ids), dim)) * (rng.random((len(ids), dim)) < np.minimum(1.0, 30.0 / mult)[:, None])
    terms = np.zeros((N_ROWS, dim), np.int64)
    np.add.at(terms, ids, np.abs(g))
    assert terms.max() <= 60 and (g[ids == HOT] != 0).any(axis=1).mean() > 0.5
    return g.astype(np.float32)


class _Run:
    def __init__(self, comm, tdt_name, dim, kind, params, idt, grads, lr, seed):
        import torch
        import wholegraph_amd.torch as wgth
        self.torch, self.wgth = torch, wgth
        self.tdt, self.dim, self.kind, self.idt, self.grads, self.lr = getattr(torch, tdt_name), dim, kind, idt, grads, lr
        self.rng = np.random.default_rng(seed)
        self.policy = wgth.create_wholememory_cache_policy(comm, memory_type="chunked", memory_location="cuda",
                                                           access_type="readwrite", ratio=RATIO)
        self.emb = wgth.create_embedding(comm, "chunked", "cpu", self.tdt, [N_ROWS, dim], cache_policy=self.policy)
        self.stride = self.emb.get_embedding_tensor().stride()[0]
        if grads is _normal_grads:
            init = self.rng.standard_normal((N_ROWS, dim)).astype(np.float32)
        else:
            init = self.rng.integers(-8, 9, (N_ROWS, dim)).astype(np.float32)
        init_t = torch.from_numpy(init).to(self.tdt)
        self.local, _ = self.emb.get_embedding_tensor().get_local_tensor(host_view=True)
        self.local.copy_(init_t)
        self.opt = wgth.create_wholememory_optimizer(self.emb, kind, params)
        padded = np.zeros((N_ROWS, self.stride), np.float32)
        padded[:, :dim] = init_t.float().numpy()
        self.tab = oracle.ShardedTable.from_full(padded, 1)
        self.tab.dim = dim
        ref_params = {k: v for k, v in params.items() if k != "grad_fold"}
        self.ref_opt = oracle.Optimizer(kind, N_ROWS, self.stride, **ref_params)
        self.model = M.RowCacheModel(N_ROWS, RATIO)
        if kind != "sgd":
            self.model.attach_states()      # (an empty cache here: the call order of the library, for the record)
        names = {"sgd": [], "adam": ["m", "v"], "adagrad": ["state_sum"], "rmsprop": ["v"]}[kind]
        self.states = [(nm, self.emb.get_optimizer_state(nm).get_local_tensor(host_view=True)[0], i * self.stride)
                       for i, nm in enumerate(names)]
        assert _info(self.emb)["slots"] == 64 * self.model.n_sets == 1024

    # bit patterns, any dtype
    def _bits(self, t):
        t = t.detach().cpu().contiguous()
        return t.view(self.torch.int32 if t.element_size() == 4 else self.torch.int16).numpy()

    def want_table(self):
        """the oracle's table in the table's dtype (16-bit tables: the one rounding of the step has been applied already)"""
        return self._bits(self.torch.from_numpy(self.tab.shards[0][:, :self.dim].copy()).to(self.tdt))

    def step(self, ids, adjust, what):
        torch = self.torch
        g = self.grads(self.rng, ids.astype(np.int64), self.dim)
        g_t = torch.from_numpy(g).to(self.tdt)
        self.emb.set_adjust_cache(adjust)
        self.emb.add_gradients(torch.from_numpy(ids).cuda(), g_t.cuda())
        self.emb.need_apply = True
        self.opt.step(self.lr)
        written_back = self.model.apply_gradients(ids, adjust)
        oracle.gradient_apply(self.tab, [self.ref_opt], [ids.astype(np.int64)], [g_t.float().numpy()], self.lr)
        if self.tdt != torch.float32:   # the one rounding to the table's dtype
            self.tab.shards[0][:, :self.dim] = torch.from_numpy(self.tab.shards[0][:, :self.dim].copy()).to(self.tdt).float().numpy()
        self.check(what)
        return written_back

    def check(self, what):
        torch = self.torch
        probe = np.concatenate([_ids(np.random.default_rng(len(what)), 0, self.idt)[:1500], np.array([HOT, 0, N_ROWS - 1], self.idt)])
        self.emb.set_adjust_cache(False)
        got = self.emb.gather(torch.from_numpy(probe).cuda())
        self.model.lookup(probe)
        want = self.want_table()
        assert self._bits(got).tobytes() == want[probe.astype(np.int64)].tobytes(), "%s: gather differs from the oracle" % what
        info = _info(self.emb)
        assert (info["occupied"], info["dirty"]) == (self.model.occupied, self.model.n_dirty), \
            "%s: occupied / dirty %d / %d, the model's %d / %d" % (what, info["occupied"], info["dirty"], self.model.occupied, self.model.n_dirty)
        torch.cuda.synchronize()
        in_table = np.ones(N_ROWS, bool)
        in_table[self.model.resident_dirty()] = False       # these lag in the raw table until their line is written back
        raw = self._bits(self.local)
        bad = np.flatnonzero((raw[in_table] != want[in_table]).any(axis=1))
        assert len(bad) == 0, "%s: %d raw rows that are not modified cache lines differ from the oracle, first %s" % (
            what, len(bad), np.flatnonzero(in_table)[bad[:5]])
        for nm, t, off in self.states:
            ref = self.ref_opt.per_element[:, off:off + self.dim].view(np.int32)
            assert np.array_equal(self._bits(t)[in_table], ref[in_table]), "%s: raw state %s differs from the oracle" % (what, nm)

    def finish(self):
        self.emb.writeback_all_cache()
        self.model.writeback()
        info = _info(self.emb)
        assert info["dirty"] == 0 and info["occupied"] == self.model.occupied
        self.torch.cuda.synchronize()
        assert self._bits(self.local).tobytes() == self.want_table().tobytes(), "raw table after write-back differs from the oracle"
        for nm, t, off in self.states:
            assert self._bits(t).tobytes() == self.ref_opt.per_element[:, off:off + self.dim].tobytes(), "state %s after write-back" % nm
        if self.kind == "adam":
            pr, _ = self.emb.get_optimizer_state("beta12t").get_local_tensor()
            assert pr.cpu().numpy().tobytes() == self.ref_opt.per_row.tobytes(), "beta powers"
        self.wgth.destroy_wholememory_optimizer(self.opt)
        self.wgth.destroy_embedding(self.emb)
        self.wgth.destroy_wholememory_cache_policy(self.policy)


def _train(run):
    torch, m, emb = run.torch, run.model, run.emb
    rng = np.random.default_rng(99)
    run.step(_ids(rng, 0, run.idt), True, "step 1")
    assert m.n_dirty > 0
    emb.drop_all_cache()      # (writes the modified lines back first)
    m.drop()
    run.step(_ids(rng, 0, run.idt), False, "step 2 (every row misses)")
    assert m.occupied == 0
    ids = _ids(rng, 0, run.idt)
    emb.set_adjust_cache(True)
    got = emb.gather(torch.from_numpy(ids).cuda(), is_training=True)
    m.gather(ids, True)
    assert run._bits(got).tobytes() == run.want_table()[ids.astype(np.int64)].tobytes(), "training gather before step 3"
    run.step(ids, True, "step 3")
    assert m.n_dirty > 0
    out = run.step(_ids(rng, 1000, run.idt), True, "step 4")
    assert len(out) > 0, "step 4 is meant to push modified lines out of the cache"
    run.finish()


SGD_WD = {"weight_decay": 0.01}
FP32_CASES = [
    # dim 260 = 1040-byte lines: launch_step_opt tile_ok, vecs 65 > 32 -> step_tile_kernel<IdxT, OPT, RPS = 1, CACHED = true>; the
    # hot id: mark_long_runs + step_long4_kernel -> apply_optimizer through the cache line. The cache's wave_copy_row takes its
    # second trip (Adam's state lines: 2080 bytes, three trips)
    (260, "sgd", SGD_WD, np.int64), (260, "sgd", SGD_WD, np.int32), (260, "adam", {}, np.int64), (260, "adam", {}, np.int32),
    (260, "adagrad", {}, np.int64), (260, "rmsprop", {}, np.int64),
    # dim 516 = 2064-byte lines: three copy trips
    (516, "sgd", SGD_WD, np.int64),
    # dim 130, stride 132: no tile kernel with a cache (tile8_ok and ragged_ok need !cached) -> step_short_kernel<IdxT, OPT, 2, float, true>
    (130, "sgd", SGD_WD, np.int64), (130, "adam", {}, np.int64), (130, "rmsprop", {}, np.int64),
    # dim 129, stride 132: step_short_kernel<IdxT, OPT, 1, float, true>
    (129, "sgd", SGD_WD, np.int64),
    # dim 28 < 32: not the tile kernel -> step_short_kernel<IdxT, OPT, 2, float, true>
    (28, "adagrad", {}, np.int64),
]


@pytest.mark.parametrize("dim,kind,params,idt", FP32_CASES, ids=["%d-%s-%s" % (c[0], c[1], np.dtype(c[3]).name) for c in FP32_CASES])
def test_fp32_training_through_the_cache(gpu_env, knobs, dim, kind, params, idt):
    knobs.unset("WM_GRAD_FOLD")
    _train(_Run(gpu_env, "float32", dim, kind, params, idt, _normal_grads, 0.05, dim))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_fp32_tree_fold_through_the_cache(gpu_env, knobs, kind):
    """{"grad_fold": "tree"}: launch_tree (tree_mark / tree_fold / tree_combine -> apply_optimizer through the cache line) beside
    step_tile_kernel<..., 1, true>. Integer gradients: the tree and the ordered sum are the same fp32 value."""
    knobs.unset("WM_GRAD_FOLD")
    _train(_Run(gpu_env, "float32", 260, kind, {"grad_fold": "tree"}, np.int64, _integer_grads, 0.05, 7))


# 16-bit tables, SGD (launch_step_sgd16):
#  520: rows16, tile_ok, vecs 65 -> step_tile_kernel<IdxT, SGD, 1, true, T>, 1040-byte lines
#  256: vecs 32 -> RPS 2;  64: vecs 8 -> RPS 8
#  100 (stride 104): dim % 8 != 0 -> no long-run side, step_short_kernel<IdxT, SGD, 4, T, true> folds every run itself
#  33 (stride 40): step_short_kernel<IdxT, SGD, 1, T, true>
# ordered fold: the hot id goes through mark_long_runs + step_long4_kernel<IdxT, SGD, T>; default fold (tree) on 520: launch_tree
@pytest.mark.parametrize("tdt_name", ["float16", "bfloat16"])
@pytest.mark.parametrize("dim", [520, 256, 64, 100, 33])
def test_16bit_sgd_through_the_cache_ordered_fold(gpu_env, knobs, tdt_name, dim):
    knobs.set("WM_GRAD_FOLD", "ordered")
    _train(_Run(gpu_env, tdt_name, dim, "sgd", SGD_WD, np.int64, _normal_grads, 0.05, dim))


@pytest.mark.parametrize("tdt_name", ["float16", "bfloat16"])
@pytest.mark.parametrize("dim", [520, 100])
def test_16bit_sgd_through_the_cache_default_fold(gpu_env, knobs, tdt_name, dim):
    """the default fold of 16-bit tables is the tree: exact on gradients whose every partial sum and result the table's dtype
    holds exactly (lr = -1, wd = 0: scatter-add)"""
    knobs.unset("WM_GRAD_FOLD")
    _train(_Run(gpu_env, tdt_name, dim, "sgd", {}, np.int32 if dim == 100 else np.int64, _sparse_integer_grads, -1.0, dim))
