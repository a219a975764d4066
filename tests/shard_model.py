"""One model of everything a caller can observe of a local, unrouted, unpinned HBM table
(`ShardModel`), a seeded generator of mixed-operation sequences over its whole API
(`gen_sequence`) and the step-by-step comparison of two table-like objects (`compare_step`,
`compare_rows`).  tests/test_shard_sequence_cpu.py checks the generator and the model without a GPU;
tests/test_shard_sequence_gpu.py replays the sequences on real tables.

The model COMPOSES the per-feature models and re-derives none of them: table_model.TableModel holds
the rows and the push rules, dup_model / bag_model the repeated-key and pooled calls,
erase_model.apply the compaction, admit_model.AdmitModel the gate, and the capacity after an
inserting call is swps_grow_plan (the library's host function) of the state before it, fed the call's
bound on its new keys: n for pull / assign / restore, the distinct count nu for an inserting lookup,
the admitted count when the gate is on.

Row order.  An inserting call draws row indices from an atomic counter, so the order of the rows of
ONE call is undefined; everything else (erase compacts by erase_plan, growth and shrink keep indices)
is a function of it.  The model keeps the keys in row order plus `loose`, the number of trailing
rows whose order among themselves is not defined (the new keys of the last inserting call).
compare_step compares the prefix exactly and the loose tail as a set and then ADOPTS the other
side's order (`adopt_order`), so a later erase compacts the order the table really has.  On its own
the model uses first-occurrence order.

A table-like object (ShardModel, or the GPU test's wrapper of a real table) has
  apply(op, args) -> dict of named results, or {"error": code}
  size(), capacity(), keys(), admission(), admission_cells(), export(keys)

Expected errors.  `push_badkey` (a push naming one absent key: SWPS_E_BADKEY, the other keys'
steps applied), `lookup_pad_err` (an inserting lookup with ~0 in it: SWPS_E_BADKEY after the call's
work) and `pull_oom` (an insert past the ceiling: SWPS_E_OOM).  After `pull_oom` WHICH of the
call's new keys got the free rows is undefined: compare_step checks that the table's new tail is a
subset of the call's new keys of exactly the free size and adopts it (`adopt_oom`).  The keys left
without a row still hold a slot; include/swps.h defines exactly two calls for a table in that
state, swps_erase ("an erase after an SWPS_E_OOM repairs the table", and it ignores keys the shard
does not hold) and swps_table_reserve ("reserve after an SWPS_E_OOM repairs the table").  The
generator issues one of the two as the very next step, so no other call ever meets such a key, and
the erase (the step after the reserve, when that repaired the table) names every new key of the
overflowing call: the set of keys held is then defined again, so the rest of the sequence, which is
a function of the seed alone, means the same on the model and on the table.

Left out:
  - routed tables: every call on them is collective; tests/dist_*_check.py cover them;
  - tables pinned by an app context: their refusals are tested in test_erase_gpu.py and
    test_table_grow_gpu.py, and a pinned table accepts none of the calls that make this interesting;
  - SWPS_INIT_FLCG: its draws depend on the call order of a float LCG that is tested through twin
    tables, not through a numpy model.

Planted defects (`doctor`), each a way the library could be wrong that only a sequence shows:
  "erase_count"  erase does not restart the row count: the next insert appends after the old count
  "erase_sketch" erase clears the admission sketch
  "prune_lt"     prune tests < where the contract says <=
  "shrink_order" shrink re-compacts (re-orders) the rows it moves
  "bag_bound"    a gated lookup_bag feeds nu, not the admitted count, to the growth plan
  "dup_badkey"   push_dup on a gated table latches SWPS_E_BADKEY for a refused id
  "run_start"    a repeated-key push reuses the previous call's run_start[nu]: the last run (largest
                 key) is one entry longer when the previous repeated-key call was larger
"""
import numpy as np

import admit_model as am
import bag_model as bm
import dup_model as dm
import erase_model as em
import table_model as tm

U64 = np.uint64
EMPTY = dm.EMPTY
SEED = am.SEED
E_OOM, E_BADKEY, E_CFG, E_STATE, E_UNSUPPORTED = -1, -2, -5, -6, -7
DOCTORS = ("erase_count", "erase_sketch", "prune_lt", "shrink_order", "bag_bound", "dup_badkey", "run_start")

# (layout, D, dtype, push rule, init): what each reaches is listed in test_shard_sequence_gpu.py
CONFIGS = [("lr", 1, "f32", "adagrad", "hash"), ("lr", 1, "f64", "sgd", "zero"), ("w2v", 7, "f32", "adagrad", "hash"),
           ("w2v", 8, "f64", "adagrad", "zero"), ("w2v", 300, "f32", "adagrad", "hash")]
# two seeds per configuration for which every condition of tests/test_shard_sequence_cpu.py holds
SEEDS = {0: (3, 8), 1: (3, 7), 2: (1, 2), 3: (1, 4), 4: (6, 8)}
STEPS = 180
CAP0, CEIL = 8, 512
SIZES = (0, 1, 2, 3, 63, 64, 65, 130, 257, 700)
OPS = ("pull", "pull_h", "push", "push_h", "lookup", "push_dup", "lookup_bag", "push_bag", "erase", "erase_h",
       "prune", "shrink", "reserve", "set_max_capacity", "set_admission", "admission_decay", "cells_roundtrip",
       "assign", "export", "save_restore", "save_restore_twin")
ERROR_OPS = ("push_badkey", "lookup_pad_err", "pull_oom")
DUP_KIND = ("lookup", "lookup_pad_err", "push_dup", "lookup_bag", "push_bag")  # they share the sorted-run scratch


def cfg_id(cfg):
    return "%s-D%d-%s-%s-%s" % cfg


def cases():
    """(cfg, seed) of every sequence the GPU test replays."""
    return [(cfg, seed) for i, cfg in enumerate(CONFIGS) for seed in SEEDS[i]]


def wire_type(layout):
    """The host forms' element type: W2V fp64, LR fp32."""
    return np.float64 if layout == "w2v" else np.float32


def _default_plan():
    import swiftmpi_amd
    return swiftmpi_amd.grow_plan


class _Behind:
    """What AdmitModel needs of the table behind the gate: rows, P, T, and pull(admitted keys)."""

    def __init__(self, shard):
        self.shard = shard

    rows = property(lambda self: self.shard.t.rows)
    P = property(lambda self: self.shard.t.P)
    T = property(lambda self: self.shard.t.T)

    def pull(self, keys):
        s = self.shard
        bound = len(keys) if s._gate_bound is None else s._gate_bound
        s._insert_call([int(k) for k in keys.tolist()], bound)


class ShardModel:
    def __init__(self, cfg, capacity=CAP0, max_capacity=CEIL, plan=None, doctor=None):
        layout, D, dtype, rule, init = cfg
        assert doctor is None or doctor in DOCTORS
        self.cfg, self.init, self.doctor = cfg, init, doctor
        self.plan = plan or _default_plan()
        self.t = tm.TableModel(layout, D, dtype, tm.LR_RATE, 1e-6, rule, seed=SEED)
        self.wire = wire_type(layout)
        self.order, self.loose = [], 0
        self.cap, self.max_cap, self.growths = capacity, max_capacity, 0
        self.slots = self.plan(capacity, 0, 0, 0)[1]
        self.gate = None
        self._gate_bound = None
        self.overflow, self.oom_pool, self.oom_free = False, None, 0
        self.ghost = 0  # "erase_count": rows the counter still counts after an erase
        self.prev_dup_n = 0  # "run_start"
        self.prev_n = {}  # op -> the size of its previous call
        self.high = 0  # the most rows ever held: an insert below it reuses a freed row
        self.was_erased, self.was_refused = set(), set()
        self.events = []
        self.ev = {}

    # ---- the observers ---------------------------------------------------------------------------
    def size(self):
        return len(self.order) + self.ghost

    def capacity(self):
        return dict(capacity=self.cap, max_capacity=self.max_cap, slots=self.slots, growths=self.growths)

    def keys(self):
        return np.array(self.order, dtype=U64)

    def admission(self):
        g = self.gate
        if g is None:
            return dict(min_count=0, width=0, depth=am.DEPTH, tested=0, admitted=0, refused=0)
        return dict(min_count=g.min_count, width=g.width, depth=am.DEPTH, **g.counters())

    def admission_cells(self):
        return self.gate.cells

    def export(self, keys):
        return self.t.export(keys)

    # ---- row order -------------------------------------------------------------------------------
    def adopt_order(self, keys):
        keys = [int(k) for k in np.asarray(keys).tolist()]
        assert sorted(keys) == sorted(self.order)
        self.order, self.loose = keys, 0

    def adopt_oom(self, tail):
        """After pull_oom: `tail` are the keys of the call that got the free rows, in row order."""
        tail = [int(k) for k in np.asarray(tail).tolist()]
        assert len(tail) == self.oom_free and set(tail) <= set(self.oom_pool) and len(set(tail)) == len(tail)
        for k in self.order[len(self.order) - self.oom_free:]:
            del self.t.rows[k]
        del self.order[len(self.order) - self.oom_free:]
        self._new_rows(tail)
        self.order += tail
        self.loose, self.oom_pool = 0, None

    # ---- capacity --------------------------------------------------------------------------------
    def _move(self, new_cap):
        self.cap, self.slots = new_cap, self.plan(new_cap, 0, 0, 0)[1]
        self.growths += 1
        self.overflow = False  # a move clamps the counter and drops the slots without a row
        self.ev["moves_table"] = self.ev.get("moves_table", 0) + 1

    def _room(self, n):
        """ensure_room: before an insert bounded by n new keys."""
        rows = min(len(self.order) + self.ghost, self.cap)
        if self.max_cap and n and rows + n > self.cap:
            nc = self.plan(self.cap, self.max_cap, rows, n)[0]
            if nc > self.cap:
                self._move(nc)
                self.ev["growth"] = self.ev.get("growth", 0) + 1

    def _new_rows(self, keys):
        if not keys:
            return
        T = self.t.T
        ks = np.array(keys, dtype=U64)
        rows = tm.hash_init(SEED, ks, self.t.layout, self.t.D, T) if self.init == "hash" else \
            np.zeros((len(ks), self.t.R), dtype=T)
        self.t.assign(ks, rows)

    def _insert_call(self, new, bound, allow_oom=False):
        """One inserting call: room for `bound` keys, then the absent keys `new` (first-occurrence
        order) get rows.  -> SWPS_E_OOM or None."""
        assert all(k not in self.t.rows for k in new) and len(set(new)) == len(new)
        self._room(bound)
        free = self.cap - len(self.order) - self.ghost
        err = None
        got = new
        if len(new) > free:
            assert allow_oom, "the generator never overflows by accident"
            self.oom_pool, self.oom_free, got = list(new), free, new[:free]
            self.overflow, err = True, E_OOM
        base = len(self.order)
        self._new_rows(got)
        self.order += got
        if got:
            self.loose = len(got)
        self.ev["inserted"] = self.ev.get("inserted", 0) + len(got)
        self.ev["reinserted"] = self.ev.get("reinserted", 0) + sum(
            1 for i, k in enumerate(got) if k in self.was_erased and base + i < self.high)
        self.high = max(self.high, len(self.order))
        return err

    def _insert_distinct(self, keys, bound, allow_oom=False):
        new = [k for k in dict.fromkeys(int(x) for x in np.asarray(keys, dtype=U64).tolist())
               if k != int(EMPTY) and k not in self.t.rows]
        return self._insert_call(new, bound, allow_oom)

    def _insert_lookup(self, keys, bag=False):
        """The inserting half of lookup / lookup_bag: the gate when it is on, else every absent key."""
        keys = np.asarray(keys, dtype=U64).reshape(-1)
        uniq, _, count = dm.coalesce(keys)
        if self.gate is None:
            self._insert_distinct(uniq, len(uniq))
            return
        g = self.gate
        before = {k: g.true_count.get(k, 0) for k in uniq.tolist() if k not in self.t.rows}
        fa = g.false_admits
        self._gate_bound = len(uniq) if (bag and self.doctor == "bag_bound") else None
        adm = g.gate(keys)
        self._gate_bound = None
        admitted = set(adm.tolist())
        ev = self.ev
        ev["gate_width"] = g.width
        ev["early"] = ev.get("early", 0) + (g.false_admits - fa)
        for k in before:
            if k in admitted:
                if k in self.was_refused:
                    ev["late_admit"] = ev.get("late_admit", 0) + 1
                    self.was_refused.discard(k)
                elif before[k] == 0:
                    ev["call_admit"] = ev.get("call_admit", 0) + 1
            else:
                self.was_refused.add(k)
                ev["refused"] = ev.get("refused", 0) + 1

    def _vals_found(self, keys):
        keys = np.asarray(keys, dtype=U64).reshape(-1)
        vals = np.zeros((len(keys), self.t.P), dtype=self.t.T)
        found = np.zeros(len(keys), dtype=np.uint8)
        for i, k in enumerate(keys.tolist()):
            if k != int(EMPTY) and k in self.t.rows:
                vals[i] = self.t.rows[k][:self.t.P]
                found[i] = 1
        return vals, found

    def _out(self, vals, host):
        return vals.astype(self.wire) if host else vals

    # ---- the operations --------------------------------------------------------------------------
    def apply(self, op, args):
        self.ev = dict(op=op, rows_before=len(self.order))
        self.events.append(self.ev)
        res = getattr(self, "_op_" + op)(**args)
        self.ev["rows_after"] = len(self.order)
        if res and "error" in res:
            self.ev["error"] = res["error"]
        return res or {}

    def _op_pull(self, keys, host=False, allow_oom=False):
        keys = np.asarray(keys, dtype=U64)
        if not len(keys):
            return dict(vals=self._out(np.zeros((0, self.t.P), dtype=self.t.T), host))
        err = self._insert_distinct(keys, len(keys), allow_oom)
        if err:
            return dict(error=err)
        return dict(vals=self._out(self.t.export(keys)[:, :self.t.P], host))

    def _op_pull_h(self, keys):
        return self._op_pull(keys, True)

    def _op_pull_oom(self, keys, host=False):
        return self._op_pull(keys, host, allow_oom=True)

    def _op_push(self, keys, grads, host=False):
        keys = np.asarray(keys, dtype=U64)
        known = np.array([k in self.t.rows for k in keys.tolist()], dtype=bool)
        self.t.push(keys[known], np.asarray(grads)[known])
        return None if known.all() else dict(error=E_BADKEY)

    def _op_push_h(self, keys, grads):
        return self._op_push(keys, grads, True)

    def _op_push_badkey(self, keys, grads, host=False):
        res = self._op_push(keys, grads, host)
        assert res and res["error"] == E_BADKEY
        return res

    def _op_lookup(self, keys, insert=True, found=False, host=False):
        keys = np.asarray(keys, dtype=U64)
        self._note_dup(len(keys))
        pad = bool((keys == EMPTY).any())
        if insert and len(keys):
            self._insert_lookup(keys)
            if pad:
                return dict(error=E_BADKEY)
        vals, fnd = self._vals_found(keys)
        res = dict(vals=self._out(vals, host))
        if found:
            res["found"] = fnd
        return res

    def _op_lookup_pad_err(self, keys, host=False):
        res = self._op_lookup(keys, True, False, host)
        assert res.get("error") == E_BADKEY
        return res

    def _note_dup(self, n):
        self.ev["dup_n"], self.ev["dup_prev"] = n, self.prev_dup_n
        op = "lookup" if self.ev["op"] == "lookup_pad_err" else self.ev["op"]
        self.ev["same_prev"], self.prev_n[op] = self.prev_n.get(op, 0), n
        self._dup_prev, self.prev_dup_n = self.prev_dup_n, n

    def _op_push_dup(self, keys, grads, reduce="sum", scale=1.0, host=False):
        keys, grads = np.asarray(keys, dtype=U64), np.asarray(grads)
        self._note_dup(len(keys))
        if not len(keys):
            return None
        real = keys[keys != EMPTY]
        if self.doctor == "run_start" and self._dup_prev > len(keys) and len(real):
            last = real.max()
            p = np.nonzero(keys == last)[0][-1]
            keys = np.concatenate([keys, [last]]).astype(U64)
            grads = np.concatenate([grads.reshape(len(keys) - 1, -1), grads.reshape(len(keys) - 1, -1)[p:p + 1]])
        unknown = dm.push_dup(self.t, keys, grads, reduce, scale)
        if len(unknown) and (self.gate is None or self.doctor == "dup_badkey"):
            return dict(error=E_BADKEY)
        return None

    def _op_lookup_bag(self, keys, offsets, weights=None, mode="sum", insert=True, host=False):
        keys = np.asarray(keys, dtype=U64)
        self._note_dup(len(keys))
        nb = len(offsets) - 1
        if insert and len(keys):
            self._insert_lookup(keys, bag=True)
        vals, fnd = self._vals_found(keys)
        out = bm.pool(vals, keys != EMPTY, offsets, weights, mode) if nb else np.zeros((0, self.t.P), dtype=self.t.T)
        return dict(out=self._out(out, host))

    def _op_push_bag(self, keys, offsets, grads, weights=None, mode="sum", scale=1.0, host=False):
        keys = np.asarray(keys, dtype=U64)
        self._note_dup(len(keys))
        if not len(keys):
            return None
        unknown = bm.push_bag(self.t, keys, offsets, grads, weights, mode, scale)
        if len(unknown) and self.gate is None:
            return dict(error=E_BADKEY)
        return None

    def _erase_dead(self, dead):
        n = len(self.order)
        ndead = int(dead.sum())
        self.ev["erased"] = ndead
        if ndead == 0 and not self.overflow:
            self.ev["moves"], self.ev["survivors"] = 0, n
            return dict(n=0)
        m, src, _ = em.plan(dead)
        self.ev["moves"], self.ev["survivors"] = len(src), m
        gone = [k for k, d in zip(self.order, dead.tolist()) if d]
        self.order = [int(k) for k in em.apply(np.array(self.order, dtype=U64), dead).tolist()]
        for k in gone:
            del self.t.rows[k]
            self.was_erased.add(k)
        self.loose, self.overflow = 0, False
        if self.doctor == "erase_count":
            self.ghost += ndead
        if self.doctor == "erase_sketch" and self.gate is not None and ndead:
            self.gate.cells[:] = 0
        return dict(n=ndead)

    def _op_erase(self, keys, host=False):
        named = set(int(k) for k in np.asarray(keys, dtype=U64).tolist())
        return self._erase_dead(np.array([k in named for k in self.order], dtype=bool))

    def _op_erase_h(self, keys):
        return self._op_erase(keys, True)

    def _op_prune(self, x):
        if self.t.rule != "adagrad":
            return dict(error=E_UNSUPPORTED)
        x = np.float64(x)
        a0 = 2 * self.t.D if self.t.layout == "w2v" else 1
        dead = np.zeros(len(self.order), dtype=bool)
        for i, k in enumerate(self.order):
            acc = self.t.rows[k][a0:].astype(np.float64)
            dead[i] = bool(np.all(acc < x)) if self.doctor == "prune_lt" else bool(np.all(acc <= x))
        return self._erase_dead(dead)

    def _op_shrink(self, keys):
        if keys >= self.cap:
            return None
        target = max(keys, min(len(self.order) + self.ghost, self.cap), 1)
        if target < self.cap:
            self._move(target)
            self.ev["shrink_move"] = 1
            if self.doctor == "shrink_order":
                self.order.sort()
        return None

    def _op_reserve(self, keys):
        if keys > self.cap:
            self._move(keys)
        return None

    def _op_set_max_capacity(self, max_keys):
        if max_keys and max_keys < self.cap:
            return dict(error=E_CFG)
        self.max_cap = max_keys
        return None

    def _op_set_admission(self, min_count, width):
        self.gate = am.AdmitModel(_Behind(self), min_count, width, SEED) if min_count > 1 else None
        self.was_refused = set()
        return None

    def _op_admission_decay(self, shift):
        if self.gate is None:
            return dict(error=E_STATE)
        self.gate.decay(shift)
        return None

    def _op_cells_roundtrip(self, shift):
        """admission_cells, a scrambling decay, admission_load of the saved cells."""
        cells = self.gate.cells.copy()
        self.gate.decay(shift)
        self.gate.cells = cells.copy()
        return dict(cells=cells)

    def _op_assign(self, keys, rows):
        keys = np.asarray(keys, dtype=U64)
        if not len(keys):
            return None
        self._insert_distinct(keys, len(keys))
        self.t.assign(keys, rows)
        return None

    def _op_export(self, keys):
        keys = np.asarray(keys, dtype=U64)
        return dict(rows=self.t.export(keys) if len(keys) else np.zeros((0, self.t.R), dtype=self.t.T))

    def _op_save_restore(self):
        """swps_save, then swps_restore into the same table: an assign of every key it holds."""
        if self.order:
            self._room(len(self.order))
        return None

    def _op_save_restore_twin(self, capacity):
        """swps_save, then swps_restore into a fresh growable table of `capacity` rows that replaces
        this one: the gate is off there, its growths start again, and the whole file is one insert."""
        m = len(self.order)
        self.cap, self.max_cap, self.growths = capacity, max(CEIL, m), 0
        self.slots = self.plan(capacity, 0, 0, 0)[1]
        self.gate, self.was_refused = None, set()
        self.ghost, self.overflow = 0, False
        if m > self.cap:
            self._move(m)  # swps_restore reserves for a file that fits under the ceiling
        self.loose = m
        self.high = m
        return None


# ==== the comparison ================================================================================
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return tm.same_bits(a, b)
    return a.shape == b.shape and np.array_equal(a, b)


def compare_step(model, other, want, got, what):
    """After one step applied to both: the call's results, size, the four capacity fields, keys()
    (prefix exact, the loose tail as a set, then adopted), and the gate.  `model` is a straight
    ShardModel, `other` any table-like object; `what` opens every message."""
    assert want.get("error") == got.get("error"), "%s: error code %r, model %r" % (what, got.get("error"), want.get("error"))
    if "error" not in want:
        assert set(want) == set(got), "%s: results %s, model %s" % (what, sorted(got), sorted(want))
        for name, w in want.items():
            g = got[name]
            if isinstance(w, (int, np.integer)):
                assert int(g) == int(w), "%s: %s = %r, model %r" % (what, name, g, w)
            else:
                assert _same(g, w), "%s: %s differs from the model (%s %s against %s %s)" % (
                    what, name, np.asarray(g).dtype, np.asarray(g).shape, np.asarray(w).dtype, np.asarray(w).shape)
    assert other.size() == model.size(), "%s: size %d, model %d" % (what, other.size(), model.size())
    assert other.capacity() == model.capacity(), "%s: capacity %r, model %r" % (what, other.capacity(), model.capacity())
    gk, mk = np.asarray(other.keys(), dtype=U64), model.keys()
    assert len(gk) == len(mk), "%s: keys() holds %d keys, model %d" % (what, len(gk), len(mk))
    if model.oom_pool is not None:
        fixed = len(mk) - model.oom_free
        assert np.array_equal(gk[:fixed], mk[:fixed]), "%s: row order before the overflowing call changed" % what
        tail = gk[fixed:].tolist()
        assert len(set(tail)) == len(tail) and set(tail) <= set(model.oom_pool), \
            "%s: the rows filled by the overflowing call are not %d of its new keys" % (what, model.oom_free)
        model.adopt_oom(gk[fixed:])
    else:
        fixed = len(mk) - model.loose
        assert np.array_equal(gk[:fixed], mk[:fixed]), "%s: row order differs at row %d of the %d defined rows" % (
            what, int(np.argmax(gk[:fixed] != mk[:fixed])), fixed)
        assert np.array_equal(np.sort(gk[fixed:]), np.sort(mk[fixed:])), "%s: the last call's new keys differ" % what
        model.adopt_order(gk)
    assert other.admission() == model.admission(), "%s: admission %r, model %r" % (what, other.admission(), model.admission())
    if model.gate is not None:
        assert np.array_equal(other.admission_cells(), model.admission_cells()), "%s: the sketch cells differ" % what


def compare_rows(model, other, what):
    """export of every key the model holds against the model's rows, bit for bit."""
    ks = model.keys()
    if len(ks):
        tm.assert_rows_equal(other.export(ks), model.export(ks), model.t.layout, what)


def replay(seq, model, other, what, every=10, checkpoint=None, strict=False):
    """Apply seq to both and compare after every step (rows, and the caller's `checkpoint(where)`,
    every `every` steps and at the end).  -> None, or (step index, op, message) of the first failing
    step; strict: that step's AssertionError is raised instead."""
    for i, (op, args) in enumerate(seq):
        where = "%s step %d %s" % (what, i, op)
        try:
            compare_step(model, other, model.apply(op, args), other.apply(op, args), where)
            if (i + 1) % every == 0 or i == len(seq) - 1:
                since = i - i % every if (i + 1) % every else i + 1 - every
                compare_rows(model, other, where if every == 1 else
                             "%s (rows are compared every %d steps: they diverged in steps %d..%d)" % (where, every, max(since, 0), i))
                if checkpoint:
                    checkpoint(where)
        except AssertionError as e:
            if strict:
                raise
            return i, op, str(e)
    return None


# ==== the generator =================================================================================
def key_pool():
    """About 600 keys: the extremes, a run of consecutive integers, keys spread over the u64 range."""
    ks = np.concatenate([np.array([0, 1, 2 ** 64 - 2], dtype=U64), np.arange(1000, 1030, dtype=U64),
                         tm.gen_keys(np.random.default_rng(5), 567)])
    assert len(set(ks.tolist())) == len(ks) == 600 and int(EMPTY) not in set(ks.tolist())
    return ks


# The forms in which an operation is due (one entry per occurrence; an operation not listed is due
# three times in whatever form the draw gives it), so that every form of the issue's list occurs.
F32, F64 = np.float32, np.float64
# kind 0.05: a bag of padding only; 0.15: one key filling a whole bag; 0.5: drawn keys with an empty bag
_BAG_FORMS = [dict(mode="sum", weighted=False, kind=0.5, insert=True), dict(mode="sum", weighted=False, kind=0.15, insert=False),
              dict(mode="sum", weighted=False, kind=0.05, insert=True), dict(mode="mean", kind=0.5, insert=True),
              dict(mode="mean", kind=0.05, insert=False), dict(mode="mean", kind=0.15, insert=True),
              dict(mode="sum", weighted=True, kind=0.5, insert=True), dict(mode="sum", weighted=True, kind=0.15, insert=False),
              dict(mode="sum", weighted=True, kind=0.05, insert=False)]
DUE_FORMS = {
    "lookup": [dict(insert=True, found=True)] * 3 + [dict(insert=False, found=True)] * 2 + [dict(insert=False, found=False)],
    "push_dup": [dict(reduce="sum", scale=1.0, G=F32), dict(reduce="sum", scale=-1.0, G=F32),
                 dict(reduce="sum", scale=1.0, G=F32), dict(reduce="mean", scale=-1.0, G=F64),
                 dict(reduce="mean", scale=1.0, G=F64), dict(reduce="mean", scale=-1.0, G=F64)],
    "lookup_bag": _BAG_FORMS, "push_bag": _BAG_FORMS,
    # kind 0.1: n = 0; 0.2: absent keys only; 0.4: the last call's rows; 0.9: a share of the keys, with
    # repeats, absent keys and ~0
    "erase": [dict(kind=0.9), dict(kind=0.9), dict(kind=0.1), dict(kind=0.1)],
    "erase_h": [dict(kind=0.9), dict(kind=0.1), dict(kind=0.2), dict(kind=0.4)],
    "prune": [dict(x=False)] * 3 + [dict(x=True)] * 3,
    "shrink": [dict(keys=0)] * 3 + [dict(k=True)] * 3,
    "set_max_capacity": [dict(max_keys=0)] * 3 + [dict(k=True)] * 3,
    "set_admission": [dict(off=False, min_count=2, width=64), dict(off=False, min_count=3, width=64),
                      dict(off=False, min_count=2, width=1 << 16), dict(off=False, min_count=3, width=1 << 16),
                      dict(off=False, min_count=2, width=64), dict(off=False, min_count=3, width=1 << 16)] + [dict(off=True)] * 3,
    "admission_decay": [dict(shift=1)] * 3 + [dict(shift=32)] * 3,
}


class _Gen:
    def __init__(self, seed, cfg, plan):
        self.rng = np.random.default_rng([77, seed, CONFIGS.index(cfg)])
        self.cfg = cfg
        self.m = ShardModel(cfg, plan=plan)
        self.pool = key_pool()
        self.G = wire_type(cfg[0])
        self.errors = 0
        self.need = {"lookup": set(SIZES[:-1]), "push_dup": set(SIZES[:-1])}
        self.pool_pending = False  # a reserve repaired an overflow: the erase of its keys is still due

    # -- keys --
    def present(self):
        return np.array(self.m.order, dtype=U64)

    def absent(self):
        have = self.m.t.rows
        return np.array([k for k in self.pool.tolist() if k not in have], dtype=U64)

    def free(self):
        m = self.m
        limit = max(m.cap, m.max_cap) if m.max_cap else m.cap
        return limit - len(m.order)

    def size(self, dup=False, op=None):
        """A call size; a repeated-key call is often the largest, so every size follows a larger one."""
        if op:  # lookup, push_dup: the sizes not yet seen after a larger call of the SAME operation, descending
            below = [n for n in self.need[op] if n < self.m.prev_n.get(op, 0)]
            if below or self.need[op]:
                return max(below) if below else SIZES[-1]
        if dup and self.m.prev_dup_n < SIZES[-1] and self.rng.random() < 0.3:
            return SIZES[-1]
        return int(self.rng.choice(SIZES))

    def distinct(self, n, absent_share, cap_absent=True):
        """Up to n distinct keys, about absent_share of them absent (never more than fit)."""
        rng = self.rng
        pre, ab = self.present(), rng.permutation(self.absent())
        if self.m.gate is not None and rng.random() < 0.7:  # ids the gate refused come again
            again = np.array([k in self.m.was_refused for k in ab.tolist()], dtype=bool)
            ab = np.concatenate([ab[again], ab[~again]])
        na = min(int(round(n * absent_share)), len(ab), self.free() if cap_absent else len(ab))
        np_ = min(n - na, len(pre))
        ks = np.concatenate([ab[:na], rng.permutation(pre)[:np_]]).astype(U64)
        return rng.permutation(ks)

    def positions(self, n, absent_share, pad=False, absent_ok=True, nd=None):
        """n positions over a few distinct keys (repeats), optionally with ~0 padding mixed in."""
        rng = self.rng
        if n == 0:
            return np.zeros(0, dtype=U64)
        nd = int(min(n, nd or rng.choice([1, 2, 5, 40, 120])))
        ks = self.distinct(nd, absent_share if absent_ok else 0.0)
        if not len(ks):
            ks = self.distinct(nd, 1.0)
        if not len(ks):
            return np.full(n, EMPTY, dtype=U64)
        out = ks[rng.integers(0, len(ks), n)]
        if pad:
            out[rng.random(n) < 0.1] = EMPTY
        return out

    def grads(self, n, G=None):
        return tm.gen_grads(self.rng, n, self.m.t.P, G or self.G)

    def offsets(self, n, empty=False):
        """CSR offsets over n positions with empty bags, and sometimes one bag holding everything."""
        rng = self.rng
        if rng.random() < 0.2:
            return np.array([0, 0, n, n], dtype=np.int64)
        nb = int(rng.integers(1, 8))
        cuts = np.sort(rng.integers(0, n + 1, nb - 1)) if nb > 1 else np.zeros(0, dtype=np.int64)
        return np.concatenate([[0] * (2 if empty else 1), cuts, [n]]).astype(np.int64)

    # -- one step --
    def draw(self, op, hint=None):
        """(op, args) for `op`, or a substitute whose precondition holds.  hint: the form of the
        operation that is due (its keys are the choices below); what it leaves open is drawn."""
        rng, m = self.rng, self.m
        have = len(m.order)
        host = bool(rng.random() < 0.3)
        hint = hint or {}
        pick = lambda name, draw: hint[name] if name in hint else draw()
        if op in ("push", "push_h", "export", "push_badkey") and have == 0:
            op = "pull"
        if op == "prune" and hint.get("x") and have == 0 and m.t.rule == "adagrad":
            op = "pull"  # a threshold between accumulator values needs rows
        if op in ("admission_decay", "cells_roundtrip") and m.gate is None:
            op = "set_admission"
        if op in ("gated_lookup", "gated_lookup_bag"):
            # what follows set_admission: many absent ids at once, so that ids are refused, come again,
            # are admitted, and collide in a 64-cell sketch
            ks = self.positions(int(rng.choice(SIZES[4:])), 0.9, nd=int(rng.choice([60, 120])))
            if op == "gated_lookup":
                return "lookup", dict(keys=ks, insert=True, found=True, host=host)
            return "lookup_bag", dict(keys=ks, offsets=self.offsets(len(ks)), weights=None, mode="mean", insert=True,
                                      host=host)
        if op in ("pull", "pull_h"):
            n = min(self.size(), 257)
            return op, dict(keys=self.distinct(n, rng.choice([0.0, 0.5, 1.0])))
        if op in ("push", "push_h"):
            ks = self.distinct(min(self.size(), 257), 0.0)
            return op, dict(keys=ks, grads=self.grads(len(ks)))
        if op == "push_badkey":
            ks = self.distinct(min(max(self.size(), 2), 257), 0.0)
            ks = np.concatenate([ks, self.absent()[:1]])
            ks = rng.permutation(ks)
            return op, dict(keys=ks, grads=self.grads(len(ks)), host=host)
        if op == "pull_oom":
            ab = rng.permutation(self.absent())
            n = self.free() + int(rng.integers(1, 20))
            return op, dict(keys=ab[:n], host=host)
        if op == "lookup":
            insert = pick("insert", lambda: bool(rng.random() < 0.6))
            n = max(self.size(True, "lookup"), 1) if (hint and not insert) else self.size(True, "lookup")
            ks = self.positions(n, rng.choice([0.0, 0.5, 1.0]), pad=not insert)
            if hint and not insert:
                ks[int(rng.integers(len(ks)))] = EMPTY
            return op, dict(keys=ks, insert=insert, found=pick("found", lambda: bool(rng.random() < 0.5)), host=host)
        if op == "lookup_pad_err":
            ks = self.positions(max(self.size(True, "lookup"), 2), 0.5)
            ks[int(rng.integers(len(ks)))] = EMPTY
            return op, dict(keys=ks, host=host)
        if op == "push_dup":
            gated = m.gate is not None
            ks = self.positions(self.size(True, "push_dup"), 0.3, pad=True, absent_ok=gated)
            if have == 0 and not gated:
                ks = np.full(len(ks), EMPTY, dtype=U64)
            if "G" in hint and self.cfg[0] != "lr":
                host = False  # the device form takes either gradient type, the host form the wire type
            G = self.G if (host or self.cfg[0] == "lr") else pick("G", lambda: rng.choice([np.float32, np.float64]))
            return op, dict(keys=ks, grads=self.grads(len(ks), G), reduce=pick("reduce", lambda: str(rng.choice(["sum", "mean"]))),
                            scale=pick("scale", lambda: float(rng.choice([1.0, -1.0]))), host=host)
        if op in ("lookup_bag", "push_bag"):
            kind = pick("kind", rng.random)
            n = max(self.size(True), 2) if hint.get("kind", 1.0) < 0.2 else self.size(True)
            gated = m.gate is not None
            fwd = op == "lookup_bag"
            insert = pick("insert", lambda: bool(rng.random() < 0.6)) if fwd else False
            ok_absent = fwd or gated
            if kind < 0.1 and n:
                ks = np.full(n, EMPTY, dtype=U64)  # a bag of padding only
                off = np.array([0, n], dtype=np.int64)
            elif kind < 0.2 and n:
                one = self.distinct(1, 0.0 if have else 1.0) if (have or ok_absent) else np.full(1, EMPTY, dtype=U64)
                ks = np.full(n, one[0], dtype=U64)  # one key filling a whole bag
                off = np.array([0, 0, n], dtype=np.int64)
            else:
                ks = self.positions(n, 0.4, pad=True, absent_ok=ok_absent)
                if not fwd and have == 0 and not gated:
                    ks = np.full(len(ks), EMPTY, dtype=U64)
                off = self.offsets(n, empty=bool(hint))
            mode = pick("mode", lambda: str(rng.choice(["sum", "mean"])))
            w = rng.uniform(-2.0, 2.0, len(ks)) if (mode == "sum" and pick("weighted", lambda: rng.random() < 0.5)) else None
            if fwd:
                return op, dict(keys=ks, offsets=off, weights=w, mode=mode, insert=insert, host=host)
            G = self.G if (host or self.cfg[0] == "lr") else rng.choice([np.float32, np.float64])
            g = tm.gen_grads(rng, len(off) - 1, m.t.P, G)
            return op, dict(keys=ks, offsets=off, grads=g, weights=w, mode=mode, scale=float(rng.choice([1.0, -1.0])),
                            host=host)
        if op in ("erase", "erase_h"):
            kind = pick("kind", rng.random)
            if kind < 0.15:
                ks = np.zeros(0, dtype=U64)  # n = 0
            elif kind < 0.3:
                ks = np.concatenate([self.absent()[:int(rng.integers(1, 9))], [EMPTY]]).astype(U64)  # removes nothing
            elif kind < 0.45 and m.loose and m.loose < have:
                ks = np.array(m.order[have - m.loose:], dtype=U64)  # the last call's rows: nothing moves
            else:
                share = rng.choice([0.1, 0.3, 0.6])
                ks = rng.permutation(self.present())[:max(1, int(have * share))]
                ks = np.concatenate([ks, ks[:3], self.absent()[:2], [EMPTY]]).astype(U64)  # repeats, absent, ~0
                ks = rng.permutation(ks)
            return op, dict(keys=ks)
        if op == "prune":
            x = 0.0
            if m.t.rule != "adagrad":
                x = float(pick("x", lambda: rng.random() < 0.5))  # refused whatever the threshold
            elif pick("x", lambda: rng.random() < 0.5) and have:
                a0 = 2 * m.t.D if m.t.layout == "w2v" else 1
                mx = np.sort(np.array([float(m.t.rows[k][a0:].max()) for k in m.order]))
                mx = mx[mx > 0]  # 0.0 is the other form; every row cold: any threshold takes them all
                x = 1.0
                if len(mx):
                    i = int(rng.integers(0, len(mx)))
                    # between two rows' largest accumulators, or exactly on one (<= keeps the contract honest)
                    x = float(mx[i]) if rng.random() < 0.5 or i + 1 == len(mx) else float((mx[i] + mx[i + 1]) / 2)
            return op, dict(x=x)
        if op == "shrink":
            if hint.get("k"):
                return op, dict(keys=int(rng.choice([have + 3, m.cap + 5])))
            return op, dict(keys=int(pick("keys", lambda: rng.choice([0, have + 3, m.cap + 5]))))
        if op == "reserve":
            return op, dict(keys=int(rng.choice([m.cap // 2, m.cap + 1, min(2 * m.cap + 3, CEIL)])))
        if op == "set_max_capacity":
            if hint.get("k"):
                return op, dict(max_keys=int(rng.choice([max(m.cap, CEIL), max(m.cap, 300)])))
            return op, dict(max_keys=int(pick("max_keys", lambda: rng.choice([0, CEIL, CEIL, max(m.cap, 300)]))))
        if op == "set_admission":
            if pick("off", lambda: m.gate is not None and rng.random() < 0.3):
                return op, dict(min_count=0, width=64)
            return op, dict(min_count=int(pick("min_count", lambda: rng.choice([2, 3]))),
                            width=int(pick("width", lambda: rng.choice([64, 64, 1 << 16]))))
        if op == "admission_decay":
            return op, dict(shift=int(pick("shift", lambda: rng.choice([1, 1, 32]))))
        if op == "cells_roundtrip":
            return op, dict(shift=int(rng.choice([1, 3, 32])))
        if op == "assign":
            ks = self.distinct(min(self.size(), 257), rng.choice([0.0, 0.5, 1.0]))
            return op, dict(keys=ks, rows=tm.gen_rows(rng, len(ks), m.t.layout, m.t.D, m.t.T))
        if op == "export":
            return op, dict(keys=self.distinct(min(self.size(), 257), 0.0))
        if op == "save_restore":
            return op, {}
        if op == "save_restore_twin":
            return op, dict(capacity=int(max(1, min(m.cap // 2, 64))))
        raise ValueError(op)

    def repair(self):
        """The step after an overflow: an erase (two thirds) or a reserve that the erase follows.  The
        erase names every new key of the overflowing call besides a share of the others, so the SET of
        keys held is defined again whichever of them had got the free rows."""
        rng, m = self.rng, self.m
        if m.overflow and rng.random() > 0.67 and m.cap <= CEIL:
            self.pool_pending = True
            return "reserve", dict(keys=m.cap + 16)
        self.pool_pending = False
        others = [k for k in m.order if k not in set(m.oom_pool)]
        others = rng.permutation(np.array(others, dtype=U64))[:int(len(others) * rng.choice([0.3, 0.6, 0.9]))]
        ks = rng.permutation(np.concatenate([np.array(m.oom_pool, dtype=U64), others]).astype(U64))
        m.oom_pool = None
        return str(rng.choice(["erase", "erase_h"])), dict(keys=ks)


def gen_sequence(seed, cfg, steps=STEPS, plan=None, with_model=False):
    """`steps` (op, args) tuples, a function of (seed, cfg, steps) alone.  Every operation is due three
    times at positions drawn at random, the rest is drawn by weight; the model runs along, so the
    generator knows which keys are present, absent or refused and never overflows by accident."""
    g = _Gen(seed, cfg, plan)
    rng = g.rng
    due = [(op, {}) for op in list(OPS) * 3 + list(ERROR_OPS) * 3 if op not in DUE_FORMS] + [
        (op, dict(h)) for op, hs in DUE_FORMS.items() for h in hs]
    due = [due[i] for i in rng.permutation(len(due))]
    filler = ["pull", "lookup", "lookup", "push_dup", "push_dup", "lookup_bag", "lookup_bag", "push_bag", "push",
              "erase", "prune", "shrink", "assign", "export", "set_admission", "set_admission"]
    seq, queue = [], []
    for i in range(steps):
        if g.m.overflow or g.pool_pending:
            op, args = g.repair()
        else:
            if queue:
                want, hint = queue.pop(0)  # an operation whose precondition did not hold when it was due
            elif due and rng.random() < len(due) / max(steps - i - 4 * len(due) // 10 - 4, 1):
                want, hint = due.pop()  # spread over the sequence, and used up before it ends
            else:
                want, hint = str(rng.choice(filler)), {}
            if want in ERROR_OPS and (g.errors + 1) * 20 > steps:
                want = "lookup"
            op, args = g.draw(want, hint)
            if op != want and want in OPS + ERROR_OPS:
                queue.append((want, hint))
            if op == "set_admission" and args["min_count"] > 1:
                queue += [("gated_lookup", {}), ("gated_lookup_bag", {}), ("gated_lookup", {})]
            g.errors += op in ERROR_OPS
        g.m.apply(op, args)
        ev = g.m.ev
        if ev.get("same_prev", 0) > ev.get("dup_n", SIZES[-1]):
            g.need.get("lookup" if op == "lookup_pad_err" else op, set()).discard(ev["dup_n"])
        seq.append((op, args))
    return (seq, g.m) if with_model else seq


def coverage(seq, events):
    """The facts tests/test_shard_sequence_cpu.py asserts of a sequence, from the model's own trace."""
    ops = {}
    for op, _ in seq:
        ops[op] = ops.get(op, 0) + 1
    er = [e for e in events if "erased" in e]
    tot = lambda name, sel=lambda e: True: sum(e.get(name, 0) for e in events if sel(e))
    follows = sorted({e["dup_n"] for e in events if "dup_n" in e and e["dup_prev"] > e["dup_n"]})
    same = {op: sorted({e["dup_n"] for e in events if "dup_n" in e and e["op"] in (op, op + "_pad_err") and
                        e["same_prev"] > e["dup_n"]}) for op in ("lookup", "push_dup")}
    return dict(ops=ops, variants=variants(seq), errors=sum(ops.get(o, 0) for o in ERROR_OPS),
                growths=tot("growth"), shrink_moves=tot("shrink_move"),
                erases_moving=sum(1 for e in er if 0 < e["moves"] < e["survivors"]),
                erases_moving_none=sum(1 for e in er if e["erased"] > 0 and e["moves"] == 0),
                erases_removing_nothing=sum(1 for e in er if e["erased"] == 0),
                reinserted_into_reused_rows=tot("reinserted"), refused_then_admitted=tot("late_admit"),
                admitted_in_one_call=tot("call_admit"),
                early_admissions_width64=tot("early", lambda e: e.get("gate_width") == 64),
                sizes_after_a_larger_call=follows, sizes_after_a_larger_lookup=same["lookup"],
                sizes_after_a_larger_push_dup=same["push_dup"], rows_at_the_end=events[-1]["rows_after"] if events else 0,
                most_rows=max(e["rows_after"] for e in events))


def variants(seq):
    """How often each form of each operation occurs in a sequence (from the arguments alone)."""
    v = {}

    def hit(name, yes=True):
        if yes:
            v[name] = v.get(name, 0) + 1

    on = False
    for op, a in seq:
        k = a.get("keys")
        hit("host form", bool(a.get("host")) or op.endswith("_h"))
        if op == "lookup":
            hit("lookup insert=%s" % a["insert"])
            hit("lookup return_found", a["found"])
            hit("lookup insert=False with padding", not a["insert"] and bool((k == EMPTY).any()))
        if op == "push_dup":
            hit("push_dup %s" % a["reduce"])
            hit("push_dup scale %+d" % a["scale"])
            hit("push_dup %s grads" % np.dtype(a["grads"].dtype).name)
            hit("push_dup with padding", bool((k == EMPTY).any()))
        if op in ("lookup_bag", "push_bag"):
            off = np.asarray(a["offsets"])
            hit("%s %s%s" % (op, a["mode"], "" if a["weights"] is None else " weighted"))
            hit("%s empty bag" % op, bool((np.diff(off) == 0).any()))
            lone = [b for b in range(len(off) - 1) if off[b + 1] > off[b]]
            hit("%s bag of padding only" % op, any((k[off[b]:off[b + 1]] == EMPTY).all() for b in lone))
            hit("%s one key fills a bag" % op, any(off[b + 1] - off[b] > 1 and k[off[b]] != EMPTY and
                                                   (k[off[b]:off[b + 1]] == k[off[b]]).all() for b in lone))
        if op == "lookup_bag":
            hit("lookup_bag insert=%s" % a["insert"])
        if op in ("erase", "erase_h"):
            hit("erase n=0", len(k) == 0)
            hit("erase with repeats, absent keys and ~0", len(k) > len(set(k.tolist())) and bool((k == EMPTY).any()))
        if op == "prune":
            hit("prune(0.0)" if a["x"] == 0 else "prune(x)")
        if op == "shrink":
            hit("shrink(0)" if a["keys"] == 0 else "shrink(k)")
        if op == "set_max_capacity":
            hit("set_max_capacity(0)" if a["max_keys"] == 0 else "set_max_capacity(k)")
        if op == "set_admission":
            if a["min_count"] > 1:
                hit("set_admission min_count %d" % a["min_count"])
                hit("set_admission width %d" % a["width"])
                hit("set_admission on again", on)
            else:
                hit("set_admission off")
            on = a["min_count"] > 1
        if op == "save_restore_twin":
            on = False
        if op == "admission_decay":
            hit("admission_decay(%d)" % a["shift"])
    return v


VARIANTS = ("host form", "lookup insert=True", "lookup insert=False", "lookup return_found",
            "lookup insert=False with padding", "push_dup sum", "push_dup mean", "push_dup scale +1", "push_dup scale -1",
            "push_dup float32 grads", "push_dup with padding", "lookup_bag sum", "lookup_bag mean", "lookup_bag sum weighted",
            "push_bag sum", "push_bag mean", "push_bag sum weighted", "lookup_bag empty bag", "push_bag empty bag",
            "lookup_bag insert=True", "lookup_bag insert=False", "erase with repeats, absent keys and ~0", "prune(0.0)",
            "shrink(0)", "shrink(k)", "set_admission min_count 2", "set_admission min_count 3", "set_admission width 64",
            "set_admission width 65536", "set_admission on again", "admission_decay(1)",
            "lookup_bag bag of padding only", "lookup_bag one key fills a bag", "push_bag bag of padding only",
            "push_bag one key fills a bag", "erase n=0", "prune(x)", "set_admission off", "admission_decay(32)",
            "set_max_capacity(0)", "set_max_capacity(k)")


def coverage_gaps(cov):
    """What a sequence lacks of the conditions of tests/test_shard_sequence_cpu.py (empty: none)."""
    gaps = ["%s x%d" % (op, cov["ops"].get(op, 0)) for op in OPS + ERROR_OPS if cov["ops"].get(op, 0) < 3]
    need = dict(growths=3, shrink_moves=1, erases_moving=2, erases_moving_none=1, erases_removing_nothing=1,
                reinserted_into_reused_rows=1, refused_then_admitted=1, admitted_in_one_call=1,
                early_admissions_width64=1, rows_at_the_end=1)
    gaps += ["%s %d < %d" % (k, cov[k], v) for k, v in need.items() if cov[k] < v]
    gaps += ["%s x%d" % (v, cov["variants"].get(v, 0)) for v in VARIANTS if cov["variants"].get(v, 0) < 3]
    gaps += ["size %d never follows a larger call" % n for n in SIZES[:-1] if n not in cov["sizes_after_a_larger_call"]]
    gaps += ["size %d never follows a larger lookup" % n for n in SIZES[:-1] if n not in cov["sizes_after_a_larger_lookup"]]
    gaps += ["size %d never follows a larger push_dup" % n for n in SIZES[:-1]
             if n not in cov["sizes_after_a_larger_push_dup"]]
    if cov["most_rows"] > CEIL + 16:
        gaps.append("%d rows held" % cov["most_rows"])
    if cov["errors"] * 20 > sum(cov["ops"].values()):
        gaps.append("%d expected-error steps" % cov["errors"])
    return gaps


def with_large_calls(seq, cfg, plan=None):
    """seq with a 700-position call in front of every call that works on a key list: a call of the same
    kind for the repeated-key calls, the bags and the erases (present keys with zero gradients or
    insert=False; an inserting lookup of present keys when the gate is on; an erase of 700 keys the
    table never holds), a lookup(insert=False) for pull / assign / export.  The inserted calls change
    no state and only leave a larger layout behind in the scratch buffers.  -> (sequence, indices of the original steps)."""
    m = ShardModel(cfg, plan=plan)
    rng = np.random.default_rng(99)
    out, orig = [], []
    G = wire_type(cfg[0])
    n = SIZES[-1]
    for op, args in seq:
        have = np.array(m.order, dtype=U64)
        big = have[rng.integers(0, len(have), n)] if len(have) else np.full(n, EMPTY, dtype=U64)
        host = bool(args.get("host", False)) or op.endswith("_h")
        extra = None
        if m.overflow:
            pass  # between an overflow and its repair nothing else runs
        elif op in ("push_dup", "push", "push_h", "push_badkey"):
            extra = "push_dup", dict(keys=big, grads=np.zeros((n, m.t.P), dtype=G), reduce="sum", scale=1.0, host=host)
        elif op == "push_bag":
            extra = "push_bag", dict(keys=big, offsets=np.array([0, 1, 1, n - 1, n], dtype=np.int64),
                                     grads=np.zeros((4, m.t.P), dtype=G), weights=None, mode="sum", scale=1.0, host=host)
        elif op == "lookup_bag":
            extra = "lookup_bag", dict(keys=big, offsets=np.array([0, 300, 300, n], dtype=np.int64), weights=None,
                                       mode="mean", insert=False, host=host)
        elif op in ("erase", "erase_h", "prune"):
            # keys no sequence ever holds: nothing is removed, and the erase's key list, probe and flags are 700 long
            extra = ("erase_h" if host else "erase"), dict(keys=np.arange(1 << 40, (1 << 40) + n, dtype=U64))
        elif op in ("lookup", "lookup_pad_err") and args.get("insert", True) and m.gate is not None and len(have):
            # through the gate: every key is present, so nothing is counted, admitted or grown, and the
            # admission flags are as long as the call's distinct keys
            extra = "lookup", dict(keys=big, insert=True, found=True, host=host)
        elif op in ("lookup", "lookup_pad_err", "pull", "pull_h", "pull_oom", "export", "assign"):
            extra = "lookup", dict(keys=big, insert=False, found=True, host=host)
        if extra:
            out.append(extra)
            m.apply(*extra)
        orig.append(len(out))
        out.append((op, args))
        m.apply(op, args)
    return out, orig
