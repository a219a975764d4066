"""One table through a long stretch of its whole API: the seeded mixed-operation sequences of
tests/shard_model.py replayed on a real HBM table and compared with the composed model after EVERY
step (return values or the error code, size, the four capacity fields, keys() in row order, the
gate's counters and cells), the rows every 10 steps.  Every comparison is equality of bits or
integers; an assertion message names the configuration, the seed, the step and the operation, and
`shard_model.gen_sequence(seed, cfg)` rebuilds the sequence from them.

What the per-feature files cannot see and this one does: host state cached by one call and
refreshed by another (row count, growth bound, growths, counters, the error latch) under every order
of calls the generator draws; grow-only scratch that holds a LARGER earlier call's layout; row order
through erase, re-insert into freed rows, shrink, growth and a query.

  layout  D    dtype  rule     init   reaches
  lr      1    f32    adagrad  hash   8-B rows: the 4-B copy lanes, the thread-per-position gather
  lr      1    f64    sgd      zero   16-B rows; prune must return SWPS_E_UNSUPPORTED
  w2v     7    f32    adagrad  hash   odd D: no 16-B alignment anywhere, scalar lanes
  w2v     8    f64    adagrad  zero   16-B paths, fp64 rows converted for the queries
  w2v     300  f32    adagrad  hash   the flagship row width: 4 800-B rows, 16-B lanes

Queries (w2v): at each checkpoint a fresh twin is filled by assign with the model's keys in a
shuffled order and the model's rows; nearest (k 1 / 10 / 64, both parts, both metrics, 33 queries, an
exclusion list, candidates naming present, erased and never-seen keys) and analogy must be equal on
table and twin bit for bit: include/swps.h promises that the answer does not depend on the insertion
order, and the twin has none of the table's history.
"""
import numpy as np
import pytest
import torch

import shard_model as sm
import table_model as tm

pytestmark = pytest.mark.gpu

U64 = np.uint64
CASES = sm.cases()
IDS = ["%s-seed%d" % (sm.cfg_id(c), s) for c, s in CASES]


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).to("cuda")


def to_np(t):
    return t.cpu().numpy()


class GpuShard:
    """A real table as the table-like object of shard_model.compare_step."""

    def __init__(self, lib, cfg, tmp_path, tag="t", capacity=sm.CAP0, max_capacity=sm.CEIL):
        self.lib, self.cfg, self.path = lib, cfg, str(tmp_path / ("%s.swps" % tag))
        self.t = self.make(capacity, max_capacity)

    def make(self, capacity, max_capacity, init=None):
        layout, D, dtype, rule, cfg_init = self.cfg
        return self.lib.Table(layout, dim=D, capacity=capacity, dtype=dtype, learning_rate=tm.LR_RATE,
                              init=init or cfg_init, seed=sm.SEED, push_rule=rule, max_capacity=max_capacity)

    def close(self):
        self.t.close()

    # ---- observers ----
    def size(self):
        return self.t.size()

    def capacity(self):
        return self.t.capacity()

    def keys(self):
        return self.t.keys()

    def admission(self):
        return self.t.admission()

    def admission_cells(self):
        return self.t.admission_cells()

    def export(self, keys):
        return to_np(self.t.export(dev(keys)))

    # ---- operations ----
    def apply(self, op, args):
        try:
            return getattr(self, "_op_" + op)(**args) or {}
        except self.lib.SwpsError as e:
            return dict(error=e.code)

    def _op_pull(self, keys, host=False):
        if host:
            return dict(vals=self.t.pull_h(keys))
        return dict(vals=to_np(self.t.pull(dev(keys))))

    def _op_pull_h(self, keys):
        return self._op_pull(keys, host=True)

    _op_pull_oom = _op_pull

    def _op_push(self, keys, grads, host=False):
        if host:
            self.t.push_h(keys, grads)
        else:
            self.t.push(dev(keys), dev(grads))

    def _op_push_h(self, keys, grads):
        self.t.push_h(keys, grads)

    _op_push_badkey = _op_push

    def _op_lookup(self, keys, insert=True, found=False, host=False):
        r = self.t.lookup(keys if host else dev(keys), insert=insert, return_found=found)
        vals, fnd = r if found else (r, None)
        if not host:
            vals, fnd = to_np(vals), (None if fnd is None else to_np(fnd))
        res = dict(vals=vals)
        if found:
            res["found"] = fnd
        return res

    def _op_lookup_pad_err(self, keys, host=False):
        return self._op_lookup(keys, True, False, host)

    def _op_push_dup(self, keys, grads, reduce="sum", scale=1.0, host=False):
        if host:
            self.t.push_dup(keys, grads, reduce, scale)
        else:
            self.t.push_dup(dev(keys), dev(grads), reduce, scale)

    def _op_lookup_bag(self, keys, offsets, weights=None, mode="sum", insert=True, host=False):
        if host:
            return dict(out=self.t.lookup_bag(keys, offsets, weights, mode, insert))
        w = None if weights is None else dev(weights)
        return dict(out=to_np(self.t.lookup_bag(dev(keys), dev(offsets), w, mode, insert)))

    def _op_push_bag(self, keys, offsets, grads, weights=None, mode="sum", scale=1.0, host=False):
        if host:
            self.t.push_bag(keys, offsets, grads, weights, mode, scale)
        else:
            w = None if weights is None else dev(weights)
            self.t.push_bag(dev(keys), dev(offsets), dev(grads), w, mode, scale)

    def _op_erase(self, keys):
        return dict(n=self.t.erase(dev(keys)))

    def _op_erase_h(self, keys):
        return dict(n=self.t.erase(np.ascontiguousarray(keys, dtype=U64)))

    def _op_prune(self, x):
        return dict(n=self.t.prune(x))

    def _op_shrink(self, keys):
        self.t.shrink(keys)

    def _op_reserve(self, keys):
        self.t.reserve(keys)

    def _op_set_max_capacity(self, max_keys):
        self.t.set_max_capacity(max_keys)

    def _op_set_admission(self, min_count, width):
        self.t.set_admission(min_count, width)

    def _op_admission_decay(self, shift):
        self.t.admission_decay(shift)

    def _op_cells_roundtrip(self, shift):
        cells = self.t.admission_cells()
        self.t.admission_decay(shift)
        self.t.admission_load(cells)
        return dict(cells=cells)

    def _op_assign(self, keys, rows):
        self.t.assign(dev(keys), dev(rows))

    def _op_export(self, keys):
        return dict(rows=self.export(keys))

    def _op_save_restore(self):
        self.t.save(self.path)
        self.t.restore(self.path)

    def _op_save_restore_twin(self, capacity):
        rows = self.t.size()
        self.t.save(self.path)
        twin = self.make(capacity, max(sm.CEIL, rows))
        try:
            twin.restore(self.path)
        except self.lib.SwpsError:
            twin.close()
            raise
        self.t.close()
        self.t = twin


# ---- the queries ---------------------------------------------------------------------------------
def same_answer(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: keys differ" % (what,)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "%s: scores differ" % (what,)


def check_queries(shard, model, seed, where):
    """nearest / analogy on the table against a twin assigned in a shuffled order (module docstring)."""
    ks = model.keys()
    if shard.cfg[0] != "w2v" or not len(ks):
        return
    D = shard.cfg[1]
    rng = np.random.default_rng([41, seed, len(model.events)])
    perm = rng.permutation(len(ks))
    twin = shard.make(len(ks) + 3, 0, init="zero")
    twin.assign(dev(ks[perm]), dev(model.export(ks)[perm]))
    q = rng.normal(0, 1, (33, D)).astype(np.float32)
    excl = ks[rng.integers(0, len(ks), (33, 3))]
    excl[::4, 1] = sm.EMPTY
    pool = sm.key_pool()
    gone = np.array([k for k in sorted(model.was_erased) if k not in model.t.rows][:20], dtype=U64)
    never = np.array([2 ** 63 + 12345, 7777777], dtype=U64)
    cand = rng.permutation(np.concatenate([rng.permutation(ks)[:max(1, len(ks) // 2)], gone, never,
                                           pool[~np.isin(pool, ks)][:10]]).astype(U64))
    abc = None
    if len(ks) >= 3:
        abc = ks[np.stack([rng.choice(len(ks), 3, replace=False) for _ in range(33)])]
    try:
        for part in ("h", "v"):
            for metric in ("dot", "cos"):
                for k, lists in ((1, False), (10, False), (64, False), (1, True), (10, True), (64, True)):
                    e, c = (excl, cand) if lists else (None, None)
                    what = "%s nearest(part=%s, metric=%s, k=%d, lists=%s)" % (where, part, metric, k, lists)
                    same_answer(shard.t.nearest(q, k=k, part=part, metric=metric, exclude=e, candidates=c),
                                twin.nearest(q, k=k, part=part, metric=metric, exclude=e, candidates=c), what)
                if abc is not None:
                    same_answer(shard.t.analogy(abc, k=10, part=part, metric=metric, candidates=cand),
                                twin.analogy(abc, k=10, part=part, metric=metric, candidates=cand),
                                "%s analogy(part=%s, metric=%s)" % (where, part, metric))
    finally:
        twin.close()


# ---- the tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_sequence_equals_model(lib, gpu, tmp_path, cfg, seed):
    name = "%s seed %d" % (sm.cfg_id(cfg), seed)
    seq = sm.gen_sequence(seed, cfg, plan=lib.grow_plan)
    model, shard = sm.ShardModel(cfg, plan=lib.grow_plan), GpuShard(lib, cfg, tmp_path)
    try:
        sm.replay(seq, model, shard, name, strict=True, checkpoint=lambda where: check_queries(shard, model, seed, where))
        assert shard.size() == model.size() > 0
    finally:
        shard.close()


@pytest.mark.parametrize("case,batch", [(0, None), (6, "8")], ids=[IDS[0], IDS[6] + "-batch8"])
def test_scratch_left_by_larger_calls_changes_nothing(lib, gpu, tmp_path, monkeypatch, case, batch):
    """The sequence as generated, and again with a 700-position call that changes no state in front of
    every call on a key list (shard_model.with_large_calls: the same operation for the repeated-key
    calls, the bags and the erases; an inserting lookup of present keys before a gated inserting
    lookup; lookup(insert=False) before pull / assign / export), so that the grow-only scratch of
    those calls holds a larger layout.  Both tables equal the model after every step, so their
    states after every original step are identical; their rows are compared with each other at the
    end too.  One seed runs with SWPS_NEAREST_BATCH small, so the queries' host loop sees a tail batch."""
    cfg, seed = CASES[case]
    name = "%s seed %d" % (sm.cfg_id(cfg), seed)
    if batch:
        monkeypatch.setenv("SWPS_NEAREST_BATCH", batch)
    plan = lib.grow_plan
    seq = sm.gen_sequence(seed, cfg, plan=plan)
    fat, orig = sm.with_large_calls(seq, cfg, plan=plan)
    assert len(fat) > len(seq) + len(seq) // 2 and [fat[i][0] for i in orig] == [op for op, _ in seq]
    ma, a = sm.ShardModel(cfg, plan=plan), GpuShard(lib, cfg, tmp_path)
    mb, b = sm.ShardModel(cfg, plan=plan), GpuShard(lib, cfg, tmp_path, "fat")
    try:
        sm.replay(seq, ma, a, name + " as generated", strict=True)
        sm.replay(fat, mb, b, name + " with large calls", strict=True, every=20,
                  checkpoint=lambda where: check_queries(b, mb, seed, where))
        assert a.size() == b.size() and a.capacity() == b.capacity() and a.admission() == b.admission()
        ks = np.sort(a.keys())
        assert np.array_equal(ks, np.sort(b.keys()))
        if len(ks):
            assert tm.same_bits(a.export(ks), b.export(ks))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("doctor", sm.DOCTORS)
def test_table_disagrees_with_every_planted_defect(lib, gpu, tmp_path, doctor):
    """The comparison has teeth on the GPU side too: against a model with one planted defect
    (tests/shard_model.py) the real table fails the replay of one of the first two sequences, at a
    step the message names.  tests/test_shard_sequence_cpu.py shows the same against the straight
    model; this shows that it is the TABLE that sides with the straight model."""
    bad = None
    for cfg, seed in CASES[:2]:
        seq = sm.gen_sequence(seed, cfg, plan=lib.grow_plan)
        shard = GpuShard(lib, cfg, tmp_path)
        try:
            bad = sm.replay(seq, sm.ShardModel(cfg, plan=lib.grow_plan, doctor=doctor), shard,
                            "%s seed %d against %r" % (sm.cfg_id(cfg), seed, doctor))
        finally:
            shard.close()
        if bad:
            print("first failing step %d (%s): %s" % bad)
            break
    assert bad, "the table agrees with the %r defect on every step" % doctor
