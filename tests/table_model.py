"""A NumPy model of the HBM parameter shard (swiftmpi_amd/csrc/swps_table.hip) and the
input generator of tests/test_table_model_gpu.py (checked on the CPU by
tests/test_table_model_cpu.py).

The library is built with -ffp-contract=off, and every push step is a chain of single
IEEE operations (fp64 add, multiply, divide, sqrt for W2V rows, then one cast to the
table type T; the same chain in T for LR rows).  NumPy runs the same operations with
the same roundings, so the model is bit-exact: every comparison is `same_bits`.

  W2V row  [h | v | h2 | v2]   (4 D elements of T; a pull returns [h | v])
  LR  row  [w | g2]            (a pull returns [w])
"""
import math

import numpy as np

U64 = np.uint64
DT = {"f32": np.float32, "f64": np.float64}


# ---- hash init (k_init_rows) --------------------------------------------------------------
def _keys(keys):
    """Keys as a uint64 array (a list of Python ints above 2^63 must not pass through float64)."""
    if isinstance(keys, np.ndarray):
        return keys.astype(U64)
    return np.array(list(keys), dtype=U64)


def splitmix64(x):
    """swps_internal.h splitmix64 on a uint64 array (arithmetic mod 2^64)."""
    x = np.asarray(x, dtype=U64) + U64(0x9e3779b97f4a7c15)
    x = (x ^ (x >> U64(30))) * U64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> U64(27))) * U64(0x94d049bb133111eb)
    return x ^ (x >> U64(31))


def unit_hash(seed, key, i):
    """unit_hash: the top 24 bits of the mixed word as a float in [0, 1) (both factors and
    the product are exact in fp32)."""
    key, i = np.asarray(key, dtype=U64), np.asarray(i, dtype=U64)
    z = splitmix64(U64(seed) ^ splitmix64(key + U64(0x632be59bd9b4e019) * (i + U64(1))))
    return (z >> U64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def hash_init(seed, keys, layout, D, T):
    """Rows [n][R] of new keys on an SWPS_INIT_HASH table: W2V (T)((double(u) - 0.5) / D) for
    e < 2D, LR unit_hash(seed, key, 0) at e == 0, zero elsewhere."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    if layout == "lr":
        out = np.zeros((len(keys), 2), dtype=T)
        out[:, 0] = unit_hash(seed, keys, np.zeros(1, dtype=U64)).astype(T)
        return out
    out = np.zeros((len(keys), 4 * D), dtype=T)
    u = unit_hash(seed, keys[:, None], np.arange(2 * D, dtype=U64)[None, :])
    out[:, :2 * D] = ((u.astype(np.float64) - 0.5) / np.float64(D)).astype(T)
    return out


# ---- the push rules -----------------------------------------------------------------------
def cfg_consts(lr, fudge):
    """The table's float32 config values (fudge 0 means 1e-6f)."""
    lr, fudge = np.float32(lr), np.float32(fudge)
    if fudge == 0:
        fudge = np.float32(1e-6)
    return lr, fudge


def w2v_step64(x, x2, a, lr, fudge, rule, reassoc=False):
    """One source's step of k_push_w2v on fp64 arrays, before the cast to T: returns
    (x', x2') in fp64.  lr, fudge: the float32 config values promoted to double.
    reassoc: the doctored a * (lr / sqrt(..)) instead of (a * lr) / sqrt(..)."""
    lr, fudge = np.float64(lr), np.float64(fudge)
    if rule == "sgd":
        return x + a * lr, x2
    x2n = x2 + a * a
    if reassoc:
        return x + a * (lr / np.sqrt(x2n + fudge)), x2n
    return x + (a * lr) / np.sqrt(x2n + fudge), x2n


def w2v_push_rows(rows, grads, lr, fudge, rule, reassoc=False, keep64=False):
    """rows [n][4D] (T, or fp64 when the caller keeps intermediates unrounded), grads
    [n][2D] in the wire type G: the rows after one push, rounded to rows.dtype."""
    T = rows.dtype
    D = rows.shape[1] // 4
    a = grads.astype(np.float64)  # the wire type promoted to fp64 (exact)
    x = rows[:, :2 * D].astype(np.float64)
    x2 = rows[:, 2 * D:].astype(np.float64)
    xn, x2n = w2v_step64(x, x2, a, lr, fudge, rule, reassoc)
    out = np.empty_like(rows, dtype=np.float64 if keep64 else T)
    out[:, :2 * D] = xn
    out[:, 2 * D:] = x2n
    return out


def lr_push_rows(rows, grads, lr, fudge, rule, reassoc=False):
    """k_push_lr: every operation in T.  rows [n][2], grads [n] fp32."""
    T = rows.dtype.type
    lr, fudge = T(lr), T(fudge)
    m = grads.reshape(-1).astype(T)
    out = rows.copy()
    if rule == "sgd":
        out[:, 0] = rows[:, 0] + lr * m
        return out
    g2 = rows[:, 1] + m * m
    out[:, 1] = g2
    if reassoc:
        out[:, 0] = rows[:, 0] + lr * (m / np.sqrt(g2 + fudge))
    else:
        out[:, 0] = rows[:, 0] + (lr * m) / np.sqrt(g2 + fudge)
    return out


class TableModel:
    """dict key -> row (table dtype).  `doctor`: None, or one of the deliberately wrong
    variants the CPU test tells apart from the true model: "reverse" (sources applied in
    reverse order), "noround" (no rounding to T between sources), "reassoc"."""

    def __init__(self, layout, dim=1, dtype="f32", learning_rate=0.7, fudge=1e-6, rule="adagrad", seed=0,
                 doctor=None):
        self.layout, self.D, self.T = layout, (dim if layout == "w2v" else 1), DT[dtype]
        self.R = 4 * self.D if layout == "w2v" else 2
        self.P = 2 * self.D if layout == "w2v" else 1
        self.lr, self.fudge = cfg_consts(learning_rate, fudge)
        self.rule, self.seed, self.doctor = rule, seed, doctor
        self.rows = {}

    def size(self):
        return len(self.rows)

    def assign(self, keys, rows):
        rows = np.asarray(rows, dtype=self.T)
        for k, r in zip(_keys(keys).tolist(), rows):
            self.rows[k] = r.copy()

    def pull(self, keys):
        """find-or-insert with hash init; the pull values [n][P]."""
        keys = _keys(keys)
        new = [k for k in dict.fromkeys(keys.tolist()) if k not in self.rows]
        if new:
            self.assign(new, hash_init(self.seed, np.array(new, dtype=U64), self.layout, self.D, self.T))
        return self.export(keys)[:, :self.P]

    def export(self, keys):
        return np.stack([self.rows[k] for k in _keys(keys).tolist()]).astype(self.T)

    def _step(self, rows, grads, keep64=False):
        re = self.doctor == "reassoc"
        if self.layout == "lr":
            return lr_push_rows(rows, grads, self.lr, self.fudge, self.rule, re)
        return w2v_push_rows(rows, grads, self.lr, self.fudge, self.rule, re, keep64)

    def push(self, keys, grads):
        """One source: distinct known keys, one step per row."""
        keys = _keys(keys)
        assert len(set(keys.tolist())) == len(keys)
        if len(keys):
            self.assign(keys, self._step(self.export(keys), np.asarray(grads)))

    def push_sources(self, keys, grads, src_counts):
        """The sources' pushes concatenated in rank order (keys distinct within a source):
        one step per source, in rank order, the row rounded to T after each."""
        keys, grads = _keys(keys), np.asarray(grads)
        grads = grads.reshape(len(keys), -1)
        off = np.concatenate([[0], np.cumsum(np.asarray(src_counts, dtype=np.int64))])
        spans = [(int(off[r]), int(off[r + 1])) for r in range(len(src_counts))]
        if self.doctor == "reverse":
            spans = spans[::-1]
        if self.doctor == "noround" and self.layout == "w2v":
            acc = {}  # rows kept in fp64 across the sources, rounded once at the end
            for a, b in spans:
                if a == b:
                    continue
                ks = keys[a:b].tolist()
                cur = np.stack([acc.get(k, self.rows[k].astype(np.float64)) for k in ks])
                nxt = self._step(cur, grads[a:b], keep64=True)
                for k, r in zip(ks, nxt):
                    acc[k] = r
            for k, r in acc.items():
                self.rows[k] = r.astype(self.T)
            return
        for a, b in spans:
            self.push(keys[a:b], grads[a:b])


# ---- a scalar restatement (Python floats, math.sqrt) for the CPU test --------------------------
def _round(x, T):
    return float(np.float32(x)) if T is np.float32 else float(x)


def scalar_w2v_row(row, grads_per_source, lr, fudge, rule, T):
    """One W2V row pushed by its sources in order, element by element with Python floats."""
    D = len(row) // 4
    lr, fudge = float(lr), float(fudge)
    out = [float(x) for x in row]
    for g in grads_per_source:
        for e in range(2 * D):
            a = float(g[e])
            if rule == "sgd":
                out[e] = _round(out[e] + a * lr, T)
                continue
            x2n = out[2 * D + e] + a * a
            out[e] = _round(out[e] + (a * lr) / math.sqrt(x2n + fudge), T)
            out[2 * D + e] = _round(x2n, T)
    return np.array(out, dtype=T)


def scalar_lr_row(row, grads_per_source, lr, fudge, rule, T):
    """One LR row, every operation rounded to T (a Python float holds every fp32 value, and
    an fp64 sum / product / quotient / root of fp32 values rounded to fp32 equals the fp32
    operation: 53 >= 2 * 24 + 2 bits)."""
    lr, fudge = float(T(lr)), float(T(fudge))
    w, g2 = float(row[0]), float(row[1])
    for m in grads_per_source:
        m = float(T(m))
        if rule == "sgd":
            w = _round(w + _round(lr * m, T), T)
            continue
        g2 = _round(g2 + _round(m * m, T), T)
        step = _round(lr * m, T)
        w = _round(w + _round(step / _round(math.sqrt(_round(g2 + fudge, T)), T), T), T)
    return np.array([w, g2], dtype=T)


# ---- comparison ------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def assert_rows_equal(got, want, layout="w2v", what=""):
    """Bit equality of exported rows, reported per quarter [h | v | h2 | v2] (LR: [w | g2])."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    names = ("h", "v", "h2", "v2") if layout == "w2v" else ("w", "g2")
    q = got.shape[1] // len(names)
    bad = []
    for i, name in enumerate(names):
        g, w = bits(got[:, i * q:(i + 1) * q]), bits(want[:, i * q:(i + 1) * q])
        if not np.array_equal(g, w):
            r, e = np.argwhere(g != w)[0]
            bad.append("%s: %d of %d elements differ, first at row %d element %d: got %r, model %r"
                       % (name, int((g != w).sum()), g.size, r, e, got[r, i * q + e], want[r, i * q + e]))
    assert not bad, "%s rows are not bit-equal to the model: %s" % (what, "; ".join(bad))


# ---- the input generator of the GPU tests ------------------------------------------------------
def gen_keys(rng, n):
    """n distinct keys spread over the u64 range (never the empty key ~0)."""
    k = np.unique(rng.integers(0, 2 ** 64 - 1, size=2 * n + 8, dtype=np.uint64))
    return rng.permutation(k)[:n]


def gen_rows(rng, n, layout, D, T):
    """Rows to assign: values around the init scale, non-zero random second-moment sums."""
    if layout == "lr":
        return np.stack([rng.uniform(-1, 1, n), rng.uniform(0.01, 3.0, n)], axis=1).astype(T)
    x = rng.uniform(-0.5, 0.5, (n, 2 * D))
    x2 = rng.uniform(0.01, 3.0, (n, 2 * D))
    return np.concatenate([x, x2], axis=1).astype(T)


def gen_grads(rng, n, width, G):
    """Mean gradients [n][width] in the wire type: magnitudes 1e-2 .. 1 with random signs,
    about 2 % exact zeros and 1 % around 1e3.  In a W2V push (width > 1) column 0 is never
    zero, so every row has an element whose step depends on every source that pushes it; an
    LR push (width 1) keeps its zeros: a zero gradient must leave the weight bit-identical
    under SGD and add 0 / sqrt(g2 + fudge) under AdaGrad."""
    g = 10.0 ** rng.uniform(-2, 0, (n, width)) * rng.choice([-1.0, 1.0], (n, width))
    u = rng.random((n, width))
    g[u < 0.01] *= 1e3
    zero = (u > 0.98)
    if width > 1:
        zero[:, 0] = False
    g[zero] = 0.0
    return g.astype(G)


def gen_sources(rng, keys, world, single=False):
    """Per-source key lists (distinct within a source) over `keys`:
      - a third of the keys in one source only, a third in two, a third in every non-empty source;
      - world 5: source 3 is empty (at world 2 an empty source would leave one source, which is
        the `single` case: only source 1 of `world` is non-empty, the distinct path);
      - source 0 lists its keys in ascending position, the last non-empty source in descending
        position (opposite orders on the shared keys), every other source shuffled.
    Returns (concatenated keys, src_counts, the keys pushed by two or more sources)."""
    n = len(keys)
    if single:
        src = [[] for _ in range(world)]
        src[1] = list(rng.permutation(n))
    else:
        live = [r for r in range(world) if not (world == 5 and r == 3)]
        src = [[] for _ in range(world)]
        for i in range(n):
            kind = i % 3
            if kind == 0:
                who = [live[int(rng.integers(len(live)))]]
            elif kind == 1:
                who = list(rng.choice(live, 2, replace=False))
            else:
                who = live
            for r in who:
                src[r].append(i)
        for r in live[1:-1]:
            src[r] = list(rng.permutation(src[r]))
        src[live[0]] = sorted(src[live[0]])
        src[live[-1]] = sorted(src[live[-1]], reverse=True)
    counts = np.array([len(s) for s in src], dtype=np.uint64)
    idx = np.array([i for s in src for i in s], dtype=np.int64)
    times = np.bincount(idx, minlength=n)
    return keys[idx], counts, keys[times >= 2]


# ---- the cases of the GPU tests (the CPU test runs the model on exactly these) -----------------
LR_RATE = 0.7
WORLDS = [2, 3, 5]
N_SINGLE = 150  # 38 blocks of 4 waves
LR_SINGLE_N = 3000
SERVED_N = 150
SERVED_EXTRA = 10  # rows no source touches
LR_SERVED_N = 3000
MODES = {"fast": ("f32", "f32"), "parity": ("f32", "f64"), "f64": ("f64", "f64")}
# D: the form fast mode (f32 rows, f32 payload) selects; parity and f64 tables take
# k_push_w2v_multi<T, double, E> at every D the context accepts
SERVED_FORMS = {1: "refused", 3: "refused", 4: "multi-E4", 5: "refused", 8: "multi-E4", 64: "multi-E4",
                65: "refused", 257: "refused (slice nch 1, tail 1, misaligned)", 260: "slice nch 1, tail 4",
                300: "slice nch 1, tail 44", 320: "slice nch 1, tail 64", 321: "refused (tail 65)",
                512: "multi-E4 (tail 0), 2 trips", 516: "slice nch 2, tail 4", 576: "slice nch 2, tail 64",
                772: "slice nch 3, tail 4", 1028: "refused (nch 4)"}
SERVED_DIMS = sorted(SERVED_FORMS)
SLICE_DIMS = [D for D in SERVED_DIMS if SERVED_FORMS[D].startswith("slice")]
SORT_LOGCAPS = [10, 17, 19, 21]


def context_accepts(dtype, D):
    """check_cfg of the W2V context: 16-byte rows, at most 4 chunks of 64 lanes."""
    E = 4 if dtype == "f32" else 2
    return D % E == 0 and D // E <= 256


def single_case(layout, D, dtype, rule, n, gtype=np.float64):
    """The inputs of one single-source case: n keys, the rows to assign, and two pushes of a
    shuffled two thirds of the keys, each (positions, gradients in the wire type)."""
    rng = np.random.default_rng([2, layout == "lr", D, dtype == "f64", rule == "sgd"])
    keys = gen_keys(rng, n)
    rows = gen_rows(rng, n, layout, D, DT[dtype])
    width = 2 * D if layout == "w2v" else 1
    pushes = []
    for _ in range(2):
        sub = rng.permutation(n)[:(2 * n) // 3]
        pushes.append((sub, gen_grads(rng, len(sub), width, gtype)))
    return dict(keys=keys, rows=rows, pushes=pushes)


def served_case(layout, dtype, gtype, D, world, single=False, n=None):
    """The inputs of one served case: n served keys and SERVED_EXTRA untouched ones with
    assigned rows, the sources' key lists, and the gradients of two (D < 16: 24) pushes in
    the wire type."""
    n = n or (SERVED_N if layout == "w2v" else LR_SERVED_N)
    rng = np.random.default_rng([3, layout == "lr", dtype == "f64", gtype == "f64", D, world, int(single)])
    keys = gen_keys(rng, n + SERVED_EXTRA)
    rows = gen_rows(rng, len(keys), layout, D, DT[dtype])
    skeys, counts, hot = gen_sources(rng, keys[:n], world, single)
    width = 2 * D if layout == "w2v" else 1
    # narrow rows get more pushes: a row of 4 D elements must hold a difference under every
    # doctoring of the CPU test, and a re-associated fp64 step differs in about one element in
    # thirty (measured on these inputs), so a hot row needs some hundreds of element steps
    npush = 24 if layout == "w2v" and D < 16 else 2
    grads = [gen_grads(rng, len(skeys), width, DT[gtype]) for _ in range(npush)]
    return dict(layout=layout, dtype=dtype, D=D, lr=LR_RATE, keys=keys, rows=rows, skeys=skeys, counts=counts,
                hot=hot, grads=grads, world=world)


def sort_case_per(logcap):
    """Keys per source of a sort-configuration case."""
    return min((1 << logcap) // 2, 30000)


def sort_case_grads(logcap):
    """The LR gradients of a sort-configuration case: three sources of sort_case_per keys."""
    return gen_grads(np.random.default_rng([4, logcap, 1]), 3 * sort_case_per(logcap), 1, np.float32)
