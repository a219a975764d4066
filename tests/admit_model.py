"""A NumPy model of admission by count on the HBM table (swiftmpi_amd/csrc/swps_admit.h, DESIGN.md
section 16; the rule is stated in include/swps.h) on top of tests/table_model.py and
tests/dup_model.py, and the fixed inputs of tests/test_admit_gpu.py (checked on the CPU by
tests/test_admit_cpu.py).

An inserting lookup on a table with admission on, with U the distinct non-padding keys of the call
in first-occurrence order and c[u] their occurrence counts:
  1. A0 = the keys of U the table lacks;
  2. ADD   cells[j][cell(j, key)] = min(2^32 - 1, cells[...] + min(c[u], min_count)) for every key
           of A0 and j = 0..3: np.add.at in u64, clipped;
  3. TEST  est(key) = min_j cells[j][cell(j, key)] over the FINISHED cells; admitted iff
           est >= min_count;
  4. the admitted keys are inserted in first-occurrence order (a dict keeps it);
  5. a refused key reads as a zero row, found = 0;
  6. tested += |A0|, admitted, refused.
cell(j, key) = fmix64(key ^ fmix64(seed + j)) & (width - 1).  Everything is integer arithmetic.

`doctor="perkey"` is the deliberately different rule the CPU test tells apart: every key of A0, in
first-occurrence order, adds its own count and is tested at once, before the later keys of the
call have added theirs.
"""
import numpy as np

import dup_model as dm
import table_model as tm

U64 = np.uint64
DEPTH = 4
SAT = 0xFFFFFFFF
EMPTY = dm.EMPTY
SEED = 11  # the tables' cfg.seed in the GPU tests


def fmix64(x):
    """swps_internal.h fmix64 on a uint64 array (arithmetic mod 2^64)."""
    x = np.asarray(x, dtype=U64).copy()
    x ^= x >> U64(33)
    x *= U64(0xff51afd7ed558ccd)
    x ^= x >> U64(33)
    x *= U64(0xc4ceb9fe1a85ec53)
    x ^= x >> U64(33)
    return x


def cell_cols(keys, seed, width):
    """[DEPTH][n] column of every key in every row of the sketch."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    with np.errstate(over="ignore"):
        salt = fmix64(U64(seed) + np.arange(DEPTH, dtype=U64))
    return (fmix64(keys[None, :] ^ salt[:, None]) & U64(width - 1)).astype(np.int64)


class AdmitModel:
    """A TableModel (`table`: hash init, its rows in insertion order) behind the gate."""

    def __init__(self, table, min_count, width, seed=SEED, doctor=None):
        assert min_count > 1 and width & (width - 1) == 0 and 64 <= width <= 1 << 30
        self.table, self.min_count, self.width, self.seed, self.doctor = table, int(min_count), int(width), seed, doctor
        self.cells = np.zeros((DEPTH, width), dtype=np.uint32)
        self.tested = self.admitted = self.refused = 0
        self.true_count = {}  # key -> clipped occurrences accumulated while absent (no sketch: exact)
        self.false_admits = 0  # admitted keys whose true count was still below min_count
        self.last_admitted = np.zeros(0, dtype=U64)

    def _add(self, keys, inc):
        cols = cell_cols(keys, self.seed, self.width)
        wide = self.cells.astype(U64)
        for j in range(DEPTH):
            np.add.at(wide[j], cols[j], inc.astype(U64))
        self.cells = np.minimum(wide, U64(SAT)).astype(np.uint32)

    def _est(self, keys):
        cols = cell_cols(keys, self.seed, self.width)
        return np.min(np.stack([self.cells[j][cols[j]] for j in range(DEPTH)]), axis=0)

    def gate(self, keys):
        """Steps 1-4 and 6 for one call's ids; returns the admitted keys in first-occurrence order."""
        uniq, _, count = dm.coalesce(keys)
        absent = np.array([k not in self.table.rows for k in uniq.tolist()], dtype=bool)
        a0, c0 = uniq[absent], np.minimum(count[absent], self.min_count).astype(np.uint32)
        if self.doctor == "perkey":
            ok = np.zeros(len(a0), dtype=bool)
            for i in range(len(a0)):
                self._add(a0[i:i + 1], c0[i:i + 1])
                ok[i] = self._est(a0[i:i + 1])[0] >= self.min_count
        else:
            if len(a0):
                self._add(a0, c0)
            ok = self._est(a0) >= self.min_count if len(a0) else np.zeros(0, dtype=bool)
        for k, c, o in zip(a0.tolist(), c0.tolist(), ok.tolist()):
            tc = self.true_count[k] = self.true_count.get(k, 0) + c
            assert o or tc < self.min_count, "a count-min sketch never under-counts"
            if o and tc < self.min_count:
                self.false_admits += 1
        adm = a0[ok]
        self.tested += len(a0)
        self.admitted += len(adm)
        self.refused += len(a0) - len(adm)
        if len(adm):
            self.table.pull(adm)
        self.last_admitted = adm
        return adm

    def lookup(self, keys, insert=True):
        """(vals [n][P] in the table dtype, found [n] uint8) of swps_lookup."""
        keys = np.asarray(keys, dtype=U64).reshape(-1)
        if insert:
            self.gate(keys)
        vals = np.zeros((len(keys), self.table.P), dtype=self.table.T)
        found = np.zeros(len(keys), dtype=np.uint8)
        for i, k in enumerate(keys.tolist()):
            if k != int(EMPTY) and k in self.table.rows:
                vals[i] = self.table.rows[k][:self.table.P]
                found[i] = 1
        return vals, found

    def decay(self, shift):
        assert 1 <= shift <= 32
        self.cells = np.zeros_like(self.cells) if shift == 32 else self.cells >> np.uint32(shift)
        # the exact counts age with the cells: (a + b) >> s >= (a >> s) + (b >> s), so "never under-counts" still holds
        self.true_count = {k: (0 if shift == 32 else v >> shift) for k, v in self.true_count.items()}

    def counters(self):
        return dict(tested=self.tested, admitted=self.admitted, refused=self.refused)

    def keys(self):
        return np.array(list(self.table.rows), dtype=U64)


# ---- the fixed inputs of the GPU tests ---------------------------------------------------------
NUS = (1, 255, 257, 5000)  # distinct keys per call: the edges of the 256-thread blocks and of the scan
MIN_COUNTS = (2, 5)
WIDTHS = (64, 1 << 16)
LAYOUTS = (("lr", 1, "f32"), ("w2v", 8, "f32"), ("w2v", 3, "f64"))
# The generator's salt, chosen so that at width 2^16 no case has a false admit (with some 7 000 keys
# in 4 x 2^16 cells about one is expected at nu = 5000; tests/test_admit_cpu.py asserts the zero), so
# the wide sketch shows the exact rule and the 64-cell one the collisions.
SALT = 2


def stream_case(nu, min_count):
    """min_count + 1 calls of exactly `nu` distinct keys each, repeats and ~0 padding shuffled in:
      once   a quarter of the keys (at least one), ONE occurrence in every call: admitted on call
             number min_count, never earlier without a collision;
      hot    a quarter, min_count .. min_count + 2 occurrences in the first call (admitted there)
             and one occurrence afterwards (present: untouched by the gate);
      rest   drawn afresh per call from a pool of twice their number, 1 .. 3 occurrences: keys that
             come and go, some admitted late, many never.
    Returns dict(calls=[ids], once=, hot=)."""
    rng = np.random.default_rng([16, nu, min_count, SALT])
    n_once = max(1, nu // 4)
    n_hot = nu // 4
    n_rest = nu - n_once - n_hot
    pool = tm.gen_keys(rng, n_once + n_hot + 2 * n_rest)
    once, hot, rest = pool[:n_once], pool[n_once:n_once + n_hot], pool[n_once + n_hot:]
    calls = []
    for c in range(min_count + 1):
        hot_m = rng.integers(min_count, min_count + 3, n_hot) if c == 0 else np.ones(n_hot, dtype=np.int64)
        sub = rng.permutation(rest)[:n_rest]
        ids = np.concatenate([once, np.repeat(hot, hot_m), np.repeat(sub, rng.integers(1, 4, n_rest)),
                              np.full(nu // 10 + 1, EMPTY, dtype=U64)])
        ids = rng.permutation(ids)
        assert len(np.unique(ids[ids != EMPTY])) == nu
        calls.append(ids)
    return dict(calls=calls, once=once, hot=hot)


def run_stream(case, min_count, width, layout="lr", D=1, dtype="f32", doctor=None):
    """The model over the case's calls -> (model, per call: vals, found, admitted keys, cells, counters)."""
    m = AdmitModel(tm.TableModel(layout, D, dtype, tm.LR_RATE, seed=SEED), min_count, width, SEED, doctor)
    trace = []
    for ids in case["calls"]:
        vals, found = m.lookup(ids)
        trace.append(dict(vals=vals, found=found, admitted=m.last_admitted, cells=m.cells.copy(), counters=m.counters()))
    return m, trace
