"""A NumPy model of the repeated-key calls (swiftmpi_amd/csrc/swps_dup.hip) on top of
tests/table_model.py, and the fixed inputs of tests/test_dup_gpu.py (checked on the CPU by
tests/test_dup_cpu.py).

The summation order is part of the ABI (include/swps.h): for a key whose occurrences are at
positions p1 < p2 < ... < pm the gradients are promoted to fp64 and, per element,
  - cut into chunks of CHUNK = 128 consecutive occurrences,
  - each chunk summed as a sequential chain that starts from its first element,
  - the chunk sums chained sequentially in chunk order, again from the first,
  - reduce = "mean": the sum divided by float64(m) once,
  - multiplied by `scale` once,
and the key takes ONE step of the table's push rule with the result (LR: rounded to fp32).
Every operation is a single IEEE operation, so the model is bit-exact.

Doctored variants (`doctor`), which the CPU test tells apart from the true model on the inputs
the GPU tests use: "nochunk" (one sequential chain over the whole run), "descending" (positions
in descending order), "zero" (chains started from 0.0), "mulmean" (mean as a multiply by 1/m).
"""
import numpy as np

import table_model as tm

CHUNK = 128
U64 = np.uint64
EMPTY = U64(0xFFFFFFFFFFFFFFFF)
NO_IDX = np.uint32(0xFFFFFFFF)
DOCTORS = ("nochunk", "descending", "zero", "mulmean")


def coalesce(keys):
    """(uniq, inv, count): the distinct keys in first-occurrence order, inv[i] = index in uniq of
    keys[i] (0xFFFFFFFF for the padding key ~0), count[u] = occurrences of uniq[u]."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    index, uniq, count = {}, [], []
    inv = np.full(len(keys), NO_IDX, dtype=np.uint32)
    for i, k in enumerate(keys.tolist()):
        if k == int(EMPTY):
            continue
        u = index.get(k)
        if u is None:
            u = index[k] = len(uniq)
            uniq.append(k)
            count.append(0)
        inv[i] = u
        count[u] += 1
    return np.array(uniq, dtype=U64), inv, np.array(count, dtype=np.uint32)


def _chain(vals, from_zero=False):
    """Sequential fp64 sum of vals[0], vals[1], ... along axis 0, from the first (or from 0.0)."""
    acc = np.zeros_like(vals[0]) if from_zero else vals[0].copy()
    for v in vals[0 if from_zero else 1:]:
        acc = acc + v
    return acc


def combine(grads, positions, reduce="sum", scale=1.0, doctor=None):
    """The combined gradient [P] (fp64) of the occurrences at `positions` of grads [n][P]."""
    pos = sorted(int(p) for p in positions)
    if doctor == "descending":
        pos = pos[::-1]
    v = np.asarray(grads)[pos].astype(np.float64)  # an fp32 input promotes exactly
    zero = doctor == "zero"
    if doctor == "nochunk":
        g = _chain(v)
    else:
        g = _chain(np.stack([_chain(v[a:a + CHUNK], zero) for a in range(0, len(v), CHUNK)]), zero)
    m = np.float64(len(pos))
    if reduce == "mean":
        g = g * (np.float64(1.0) / m) if doctor == "mulmean" else g / m
    return g * np.float64(scale)


def reduced(keys, grads, reduce="sum", scale=1.0, doctor=None):
    """(uniq, G): one combined gradient [nu][P] (fp64) per distinct key, first-occurrence order."""
    keys = np.asarray(keys, dtype=U64).reshape(-1)
    grads = np.asarray(grads).reshape(len(keys), -1)
    uniq, inv, _ = coalesce(keys)
    where = [[] for _ in uniq]
    for i, u in enumerate(inv.tolist()):
        if u != int(NO_IDX):
            where[u].append(i)
    G = np.stack([combine(grads, w, reduce, scale, doctor) for w in where]) if len(uniq) else \
        np.zeros((0, grads.shape[1]))
    return uniq, G


def push_dup(model, keys, grads, reduce="sum", scale=1.0, doctor=None):
    """swps_push_dup on a TableModel: one step per distinct key the model holds (W2V: the fp64
    gradient; LR: rounded to fp32 first); keys it lacks are skipped.  Returns the unknown keys."""
    uniq, G = reduced(keys, grads, reduce, scale, doctor)
    known = np.array([k in model.rows for k in uniq.tolist()], dtype=bool)
    if model.layout == "lr":
        G = G.astype(np.float32)
    if known.any():
        model.push(uniq[known], G[known])
    return uniq[~known]


# ---- the fixed inputs of the GPU tests ---------------------------------------------------------
# run lengths on both sides of the chunk size and of two / three chunks, one long run; 3 for the
# mean (x / 3 and x * (1 / 3) round differently); "mag" and "negz" are the special runs below
RUNS = [1, 2, 3, 127, 128, 129, 257, 385, 3000]
MAG = [1e16, 1.0, -1e16, 1.0]  # ascending: ((1e16 + 1) - 1e16) + 1 = 1; descending: 0
# Sums of fp32 gradients of these magnitudes are often EXACT in fp64, and an fp32 table or the
# LR rule's cast to fp32 hides a last-bit difference of the fp64 gradient, so column 0 of two runs
# is set by hand (all exactly representable in fp32):
#   the m = 3 run: s = (3 + 3 * 2^-24) + 2^-51; s / 3 rounds to 1 + 2^-24 + 2^-52 and to fp32
#     1 + 2^-23, s * (1 / 3) rounds to the fp32 midpoint 1 + 2^-24 and to fp32 1.0
#   the m = 257 run: zeros but 1e16 at occurrence 0 and 1, 1, -1e16 at occurrences 128..130: one
#     sequential chain gives 0, the chunk rule gives (1e16 + ((1 + 1) - 1e16)) = 2
MEAN3 = [3.0, 3 * 2.0 ** -24, 2.0 ** -51]
CHUNKY = {0: 1e16, 128: 1.0, 129: 1.0, 130: -1e16}
NEGZ = 5  # a run whose gradients are all -0.0 on a row element that holds -0.0: a chain started
#           from 0.0 gives +0.0, and -0.0 + +0.0 = +0.0 where -0.0 + -0.0 = -0.0


def push_case(layout, D, dtype, gtype):
    """keys [K] with their rows, and two calls (keys [n] with repeats, grads [n][P] in gtype) whose
    positions interleave the runs at random.  Key order: RUNS, then the MAG run, then the NEGZ run."""
    rng = np.random.default_rng([13, layout == "lr", D, dtype == "f64", gtype == "f64"])
    T, G = tm.DT[dtype], tm.DT[gtype]
    P = 2 * D if layout == "w2v" else 1
    lens = RUNS + [len(MAG), NEGZ]
    keys = tm.gen_keys(rng, len(lens))
    rows = tm.gen_rows(rng, len(keys), layout, D, T)
    zcol = 1 if P > 1 else 0
    rows[-1, zcol] = T(-0.0)
    calls = []
    for _ in range(2):
        which = rng.permutation(np.repeat(np.arange(len(lens)), lens))
        g = tm.gen_grads(rng, len(which), P, G)
        g[which == len(RUNS), 0] = np.array(MAG, dtype=G)  # in position order
        g[which == len(RUNS) + 1, zcol] = G(-0.0)
        g[which == RUNS.index(3), 0] = np.array(MEAN3, dtype=G)
        col = np.zeros(257, dtype=G)
        for o, x in CHUNKY.items():
            col[o] = x
        g[which == RUNS.index(257), 0] = col
        calls.append((keys[which], g))
    return dict(layout=layout, D=D, dtype=dtype, keys=keys, rows=rows, calls=calls)


def run_case(case, rule, reduce, scale, doctor=None):
    """The exported rows of the case's keys after its two calls, by the model."""
    m = tm.TableModel(case["layout"], case["D"], case["dtype"], tm.LR_RATE, 1e-6, rule)
    m.assign(case["keys"], case["rows"])
    for k, g in case["calls"]:
        push_dup(m, k, g, reduce, scale, doctor)
    return m.export(case["keys"])
