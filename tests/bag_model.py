"""A NumPy model of the pooled calls (swiftmpi_amd/csrc/swps_bag.hip) on top of tests/table_model.py
and tests/dup_model.py, and the fixed inputs of tests/test_bag_gpu.py (checked on the CPU by
tests/test_bag_cpu.py).

Forward (include/swps.h, swps_lookup_bag): per element, in fp64 whatever the table dtype,
  term(p) = double(val(p))  or  double(val(p)) * w[p]                      one multiply
  a bag is cut into chunks of CHUNK = 128 consecutive POSITIONS; a chunk's sum is the sequential
  chain of its MEMBERS' (non-padding positions') terms in ascending position, from the first member;
  chunks without members are skipped; the chunk sums are chained in chunk order from the first
  non-empty one; mode "mean" divides once by float64(m_b); one cast to the table dtype; m_b = 0 gives
  +0.0.
Backward (swps_push_bag): term(p) = double(G[bag(p)]) (* w[p] | / float64(m_bag(p))), then exactly
dup_model.push_dup(reduce="sum", scale) of the [n][P] fp64 term matrix.
Every step is a single IEEE operation, so the model is bit-exact.

Doctored variants (`doctor`), which the CPU test tells apart from the true model on the inputs the
GPU tests use.  Forward: "onechain" (one chain per bag), "descending", "zero" (chains from 0.0),
"mulmean" (mean as a multiply by 1/m), "tacc" (accumulation in the table dtype), "padcount"
(padding counted in m_b), "w32" (the weight applied in fp32).  Backward: "keymean" (the mean's
divisor, that of the key's first bag, applied to the key's sum instead of to each term).
"""
import numpy as np

import dup_model as dm
import table_model as tm

CHUNK = dm.CHUNK
U64 = np.uint64
EMPTY = dm.EMPTY
FWD_DOCTORS = ("onechain", "descending", "zero", "mulmean", "tacc", "padcount", "w32")
BWD_DOCTORS = ("keymean",)


def _chain(terms, zero, like):
    if not len(terms):
        return None
    acc = np.zeros_like(like) if zero else terms[0].copy()
    for v in terms[0 if zero else 1:]:
        acc = acc + v
    return acc


def pool(vals, member, offsets, weights=None, mode="sum", doctor=None):
    """vals [n][P] (table dtype T): what swps_lookup returns per position; member [n] bool (False:
    padding); offsets [nbags + 1] -> the pooled rows [nbags][P] in T."""
    vals = np.asarray(vals)
    T = vals.dtype.type
    A = T if doctor == "tacc" else np.float64  # the accumulator type
    n, P = vals.shape
    off = [int(x) for x in offsets]
    assert off[0] == 0 and off[-1] == n and all(a <= b for a, b in zip(off, off[1:]))
    out = np.zeros((len(off) - 1, P), dtype=T)
    zero = doctor == "zero"
    like = np.zeros(P, dtype=A)
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        step = (hi - lo) if doctor == "onechain" else CHUNK
        sums, m = [], 0
        for a in range(lo, hi, max(step, 1)):
            pos = [p for p in range(a, min(a + step, hi)) if member[p]]
            if doctor == "descending":
                pos = pos[::-1]
            terms = []
            for p in pos:
                if weights is None:
                    v = vals[p].astype(A)
                elif doctor == "w32":
                    v = (vals[p].astype(np.float32) * np.float32(weights[p])).astype(A)
                else:
                    v = (vals[p].astype(np.float64) * np.float64(weights[p])).astype(A)
                terms.append(v)
            m += len(pos)
            s = _chain(terms, zero, like)
            if s is not None:
                sums.append(s)
        if doctor == "descending":
            sums = sums[::-1]
        if not sums:
            continue  # +0.0
        acc = _chain(sums, zero, like)
        if mode == "mean":
            mm = A(m + (0 if doctor != "padcount" else int((~np.asarray(member[lo:hi])).sum())))
            acc = acc * (A(1.0) / mm) if doctor == "mulmean" else acc / mm
        out[b] = acc.astype(T)
    return out


def lookup_vals(model, keys, insert=True):
    """(vals [n][P], member [n]) of a TableModel: the per-position pull values (an absent key with
    insert=False, and padding, read as zero rows)."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    member = keys != EMPTY
    vals = np.zeros((len(keys), model.P), dtype=model.T)
    if insert and member.any():
        model.pull(keys[member])
    for i, k in enumerate(keys.tolist()):
        if member[i] and k in model.rows:
            vals[i] = model.rows[k][:model.P]
    return vals, member


def lookup_bag(model, keys, offsets, weights=None, mode="sum", insert=True, doctor=None):
    vals, member = lookup_vals(model, keys, insert)
    return pool(vals, member, offsets, weights, mode, doctor)


def bag_of(offsets, n):
    off = np.asarray([int(x) for x in offsets], dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off)) if n else np.zeros(0, dtype=np.int64)


def expand(G, keys, offsets, weights=None, mode="sum"):
    """The fp64 [n][P] term matrix of swps_push_bag (one IEEE operation per element)."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    G = np.asarray(G)
    G = G.reshape(len(offsets) - 1, -1)
    bo = bag_of(offsets, len(keys))
    terms = G[bo].astype(np.float64)
    if weights is not None:
        terms = terms * np.asarray(weights, dtype=np.float64)[:, None]
    elif mode == "mean":
        m = np.bincount(bo[keys != EMPTY], minlength=len(offsets) - 1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = terms / m[bo][:, None]  # a padding position's term is never used
    return terms


def push_bag(model, keys, offsets, G, weights=None, mode="sum", scale=1.0, doctor=None):
    """swps_push_bag on a TableModel; returns the unknown keys."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    if doctor == "keymean" and mode == "mean":
        terms = expand(G, keys, offsets, None, "sum")
        uniq, Gk = dm.reduced(keys, terms, "sum", 1.0)
        bo = bag_of(offsets, len(keys))
        m = np.bincount(bo[keys != EMPTY], minlength=len(offsets) - 1).astype(np.float64)
        first = {}
        for i, k in enumerate(keys.tolist()):
            first.setdefault(k, i)
        div = np.array([m[bo[first[k]]] for k in uniq.tolist()])
        Gk = (Gk / div[:, None]) * np.float64(scale)
        known = np.array([k in model.rows for k in uniq.tolist()], dtype=bool)
        if model.layout == "lr":
            Gk = Gk.astype(np.float32)
        if known.any():
            model.push(uniq[known], Gk[known])
        return uniq[~known]
    return dm.push_dup(model, keys, expand(G, keys, offsets, weights, mode), "sum", scale)


# ---- the fixed inputs of the GPU tests ---------------------------------------------------------
# Column 0 of some keys' rows is set by hand (every value is exact in fp32; X = float32(1e16)):
#   MAG bag    [X, 1, -X, 1]: ascending ((X + 1) - X) + 1 = 1 (X + 1 rounds to X), descending 0
#   CHUNKY bag 257 positions of 0 but X at position 0 and 1, 1, -X at positions 128..130: one chain
#              gives ((X + 1) + 1) - X = 0, the chunk rule X + ((1 + 1) - X) = 2
#   MEAN3 bag  [3, 3 * 2^-24, 2^-51]: s / 3 and s * (1 / 3) round differently, in fp64 and after
#              the cast to fp32 (tests/dup_model.py)
#   NEGZ bag   five times a key whose element `zcol` is -0.0: a chain from 0.0 gives +0.0
#   W32 bag    one key with 1 + 2^-23 under the weight 1 + 2^-24: the fp64 product lies 2^-47 above
#              the fp32 midpoint and casts to 1 + 2^-22; float32(w) is 1.0 and gives 1 + 2^-23
X = float(np.float32(1e16))
SPECIAL = dict(Z=0.0, A=X, B=1.0, C=-X, M1=3.0, M2=3 * 2.0 ** -24, M3=2.0 ** -51, W=1.0 + 2.0 ** -23)
NAMES = list(SPECIAL) + ["NZ"]
W32_WEIGHT = 1.0 + 2.0 ** -24
LENS = [1, 2, 3, 127, 128, 129, 385, 3000]  # random bags; 0, 257 and 300 are built by hand below
NRANDOM = 40
PADK = -1  # index standing for the padding key in the bag lists


def bag_case(layout, D, dtype):
    """keys [K] with their rows; the call's ids [n] (padding: ~0), offsets [nbags + 1], fp64 weights
    [n]; `bags`: name -> bag index of the hand-built bags."""
    rng = np.random.default_rng([14, layout == "lr", D, dtype == "f64"])
    T = tm.DT[dtype]
    P = 2 * D if layout == "w2v" else 1
    K = len(NAMES) + NRANDOM
    keys = tm.gen_keys(rng, K)
    rows = tm.gen_rows(rng, K, layout, D, T)
    ix = {name: i for i, name in enumerate(NAMES)}
    for name, v in SPECIAL.items():
        rows[ix[name], 0] = T(v)
    zcol = 1 if P > 1 else 0
    rows[ix["NZ"], zcol] = T(-0.0)
    rnd = np.arange(len(NAMES), K)

    def draw(m):
        return list(rng.choice(rnd, m))  # repeats inside a bag, and the same keys across bags

    chunky = [ix["Z"]] * 257
    chunky[0], chunky[128], chunky[129], chunky[130] = ix["A"], ix["B"], ix["B"], ix["C"]
    hole = draw(128) + [PADK] * 128 + draw(44)  # 300 positions, the middle chunk all padding
    named = [("empty0", []), ("empty1", []), ("mag", [ix["A"], ix["B"], ix["C"], ix["B"]]), ("len1", draw(1)),
             ("negz", [ix["NZ"]] * 5), ("empty2", []), ("mean3", [ix["M1"], ix["M2"], ix["M3"]]), ("len2", draw(2)),
             ("pad_head", [PADK] + draw(2)), ("len127", draw(127)), ("chunky", chunky), ("len3", draw(3)),
             ("pad_mid", draw(1) + [PADK] + draw(1)), ("len128", draw(128)), ("hole", hole),
             ("only_pad", [PADK] * 4), ("len129", draw(129)), ("w32", [ix["W"]]), ("len3000", draw(3000)),
             ("pad_tail", draw(2) + [PADK]), ("len385", draw(385)), ("empty3", []), ("empty4", [])]
    assert sorted(len(b) for name, b in named if name.startswith("len")) == LENS
    flat = np.array([i for _, b in named for i in b], dtype=np.int64)
    ids = np.where(flat == PADK, EMPTY, keys[np.maximum(flat, 0)]).astype(U64)
    offsets = np.concatenate([[0], np.cumsum([len(b) for _, b in named])]).astype(np.int64)
    bags = {name: i for i, (name, _) in enumerate(named)}
    weights = rng.uniform(-2.0, 2.0, len(ids))
    weights[offsets[bags["w32"]]] = W32_WEIGHT
    return dict(layout=layout, D=D, dtype=dtype, P=P, zcol=zcol, keys=keys, rows=rows, ids=ids, offsets=offsets,
                weights=weights, bags=bags)


def case_model(case, rule="adagrad"):
    m = tm.TableModel(case["layout"], case["D"], case["dtype"], tm.LR_RATE, 1e-6, rule)
    m.assign(case["keys"], case["rows"])
    return m


def forward(case, mode="sum", weighted=False, doctor=None):
    """The pooled rows of the case by the model."""
    w = case["weights"] if weighted else None
    return lookup_bag(case_model(case), case["ids"], case["offsets"], w, mode, True, doctor)


def bag_grads(case, gtype):
    """Two bag-gradient matrices [nbags][push elems] (two chained calls: the accumulators matter)."""
    rng = np.random.default_rng([15, case["layout"] == "lr", case["D"], gtype == "f64"])
    nb = len(case["offsets"]) - 1
    return [tm.gen_grads(rng, nb, case["P"], tm.DT[gtype]) for _ in range(2)]


def backward(case, gtype, rule, mode="sum", weighted=False, scale=1.0, doctor=None):
    """The exported rows of the case's keys after its two push_bag calls, by the model."""
    m = case_model(case, rule)
    w = case["weights"] if weighted else None
    for G in bag_grads(case, gtype):
        assert len(push_bag(m, case["ids"], case["offsets"], G, w, mode, scale, doctor)) == 0
    return m.export(case["keys"])
