"""Top-k nearest-neighbour and analogy queries on the HBM table (swps_nearest / swps_analogy,
swiftmpi_amd/csrc/swps_nearest.hip) against numpy: bit for bit on integer-valued rows (every dot
product and r.r is exact in fp32 there), within a derived fp32 bound on real-valued rows, the
determinism contract (insertion order, batch size, candidate list), the error codes, and routed
tables (RCCL at world 1 here, two gloo ranks in tests/dist_nearest_check.py).  Tables are filled
with swps_assign_h; nothing is trained."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
PART = {"h": 0, "v": 1}


def _port():
    from conftest import free_port
    return free_port()


def make_keys(rng, n):
    return rng.permutation(np.arange(1, 4 * n + 1))[:n].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)


def fill(sw, D, keys, block, part, dtype, order=None, capacity=None):
    """A W2V table whose `part` block of key i is block[i]; the other blocks hold other values."""
    n = len(keys)
    rows = np.zeros((n, 4 * D))
    p = PART[part]
    rows[:, (1 - p) * D:(2 - p) * D] = 3.0 - block[::-1]
    rows[:, 2 * D:] = 7.0
    rows[:, p * D:(p + 1) * D] = block
    if order is None:
        order = np.arange(n)
    k = np.ascontiguousarray(keys[order])
    r = np.ascontiguousarray(rows[order])
    t = sw.Table("w2v", dim=D, capacity=capacity or n + 8, dtype=dtype, init="zero")
    sw.capi.check(sw.capi.lib().swps_assign_h(t.h, sw.capi.ptr(k), n, sw.capi.ptr(r)))
    return t


def int_case(D, nrows, nq, seed):
    """Integer rows in [-4, 4] with duplicated rows and a zero row, integer queries in [-12, 12]:
    |dot| <= 300 * 12 * 4 < 2^24, so fp32 sums are exact in any order."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-4, 5, (nrows, D)).astype(np.float64)
    m = min(20, nrows // 3)
    if m:
        rows[m:2 * m] = rows[:m]  # ties: the smaller key decides
    if nrows > 2:
        rows[nrows // 2] = 0
    keys = make_keys(rng, nrows)
    q = rng.integers(-12, 13, (nq, D)).astype(np.float32)
    return keys, rows, q


def f32_scores(rows, q, metric):
    """np.float32(dot) / np.sqrt(np.float32(r.r)) (0 for a zero row) on exactly representable sums.
    Non-finite rows or queries (test_non_finite_scores derives why this is the fp32 chain's value
    there too) take elementwise IEEE products and sums, not a BLAS call whose handling of inf * 0 is
    its own business."""
    q64 = q.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if np.isfinite(rows).all() and np.isfinite(q64).all():
            dot = (q64 @ rows.T).astype(np.float32)
        else:
            dot = (q64[:, None, :] * rows[None, :, :]).sum(2).astype(np.float32)
        if metric == "dot":
            return dot
        n2 = (rows * rows).sum(1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = dot / np.sqrt(n2)[None, :]
    assert s.dtype == np.float32
    return np.where(n2[None, :] == 0, np.float32(0), s)


def as_np(keys, scores):
    if hasattr(keys, "data_ptr"):
        return keys.cpu().numpy().view(np.uint64), scores.cpu().numpy()
    return keys, scores


# ---- 1. bit-exact on integer-valued rows ---------------------------------------------------
# each axis' extremes: D (1: one k step; 5: odd, scalar staging; 32: one chunk; 100: k tail; 300),
# rows (1; 31 / 33: around a wave's 32 rows; 1031: several tiles with a tail), nq (1; 33: a second
# query tile; 70), k (1; 10; 64 = the maximum, > rows for the small tables), h / v, both metrics,
# both storage types, host and device arguments
INT_CASES = [
    (1, 1, 1, 1, "v", "cos", "f32", False),
    (5, 31, 33, 64, "h", "dot", "f64", False),
    (32, 33, 70, 10, "v", "cos", "f64", True),
    (100, 1031, 33, 64, "h", "cos", "f32", False),
    (300, 1031, 70, 10, "v", "cos", "f32", True),
    (300, 1031, 1, 1, "v", "dot", "f64", False),
    (5, 1031, 70, 1, "v", "cos", "f32", False),
    (300, 33, 33, 64, "h", "cos", "f32", False),
]


@pytest.mark.parametrize("D,nrows,nq,k,part,metric,dtype,dev", INT_CASES)
def test_integer_rows_bit_exact(lib, gpu, D, nrows, nq, k, part, metric, dtype, dev):
    from swiftmpi_amd.evaluate import topk_order
    keys, rows, q = int_case(D, nrows, nq, seed=D * 7 + nrows)
    t = fill(lib, D, keys, rows, part, dtype)
    wk, ws = topk_order(f32_scores(rows, q, metric), keys, k)
    arg = torch.as_tensor(q, device=gpu) if dev else q
    gk, gs = t.nearest(arg, k=k, part=part, metric=metric)
    assert (hasattr(gk, "data_ptr") and gk.is_cuda) if dev else isinstance(gk, np.ndarray)
    gk, gs = as_np(gk, gs)
    assert gk.shape == (nq, k) and gs.dtype == np.float32
    assert np.array_equal(gk, wk)
    assert np.array_equal(gs, ws)
    if k > nrows:
        assert np.all(gk[:, nrows:] == EMPTY) and np.all(np.isneginf(gs[:, nrows:]))
    # exclusions (with an unused slot) and a candidate subset that names keys the table lacks
    rng = np.random.default_rng(1)
    excl = np.stack([rng.choice(keys, 3) for _ in range(nq)])
    excl[:, 2] = EMPTY
    cand = np.concatenate([rng.choice(keys, max(1, nrows // 2), replace=False), make_keys(rng, 5) + np.uint64(1)])
    wk, ws = topk_order(f32_scores(rows, q, metric), keys, k, excl, cand)
    gk, gs = as_np(*t.nearest(arg, k=k, part=part, metric=metric, exclude=excl, candidates=cand))
    assert np.array_equal(gk, wk)
    assert np.array_equal(gs, ws)
    t.close()


# ---- 2. the determinism contract --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_case(D, nrows=1660, nq=70, seed=3):
    rng = np.random.default_rng(seed + D)
    rows = rng.normal(0, 1, (nrows, D)).astype(np.float32).astype(np.float64)  # fp32-representable
    keys = make_keys(rng, nrows)
    q = rng.normal(0, 1, (nq, D)).astype(np.float32)
    return keys, rows, q


def test_host_query_batches(lib, gpu, monkeypatch):
    """The host's loop over query batches (SWPS_NEAREST_BATCH shrinks a batch to 32 queries: 70
    queries = 3 batches with a tail) gives what one batch gives."""
    keys, rows, q = real_case(100, 1031)
    t = fill(lib, 100, keys, rows, "v", "f32")
    rng = np.random.default_rng(9)
    excl = np.stack([rng.choice(keys, 2, replace=False) for _ in range(len(q))])
    abc = keys[np.stack([rng.choice(len(keys), 3, replace=False) for _ in range(len(q))])]
    one = t.nearest(q, k=10, exclude=excl) + t.analogy(abc, k=3)
    monkeypatch.setenv("SWPS_NEAREST_BATCH", "32")
    three = t.nearest(q, k=10, exclude=excl) + t.analogy(abc, k=3)
    for a, b in zip(one, three):
        assert np.array_equal(a, b)
    t.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_results_do_not_depend_on_order_batch_or_candidates(lib, gpu, dtype):
    D = 100
    keys, rows, q = real_case(D, 1031)
    rng = np.random.default_rng(8)
    a = fill(lib, D, keys, rows, "v", dtype)
    b = fill(lib, D, keys, rows, "v", dtype, order=rng.permutation(len(keys)), capacity=5000)
    for metric in ("cos", "dot"):
        ak, as_ = a.nearest(q, k=10, metric=metric)
        bk, bs = b.nearest(q, k=10, metric=metric)
        assert np.array_equal(ak, bk) and np.array_equal(as_, bs)  # insertion order, table capacity
        for i in (0, 31, 32, 69):  # a query alone = the same query inside the batch of 70
            k1, s1 = a.nearest(q[i:i + 1], k=10, metric=metric)
            assert np.array_equal(k1[0], ak[i]) and np.array_equal(s1[0], as_[i])
        k64, s64 = a.nearest(q, k=64, metric=metric)  # k
        assert np.array_equal(k64[:, :10], ak) and np.array_equal(s64[:, :10], as_)
        ck, cs = a.nearest(q, k=10, metric=metric, candidates=rng.permutation(keys))  # every key listed
        assert np.array_equal(ck, ak) and np.array_equal(cs, as_)
    a.close()
    b.close()


# ---- 3. real-valued rows against the fp64 reference, no case left out ------------------------
def check_against_fp64(gk, gs, s64, keys, E, allowed):
    """The four conditions, per query.  s64: fp64 scores [nq, n]; E: [nq] bounds; allowed: [nq, n]
    bool (candidate and not excluded)."""
    pos = {int(x): i for i, x in enumerate(keys)}
    for i in range(gk.shape[0]):
        assert np.all(gk[i] != EMPTY)
        idx = np.array([pos[int(x)] for x in gk[i]])
        ref = s64[i, idx]
        assert np.all(np.abs(gs[i].astype(np.float64) - ref) <= E[i]), (i, float(np.abs(gs[i] - ref).max()), E[i])
        assert np.all(gs[i, 1:] <= gs[i, :-1]) and len(set(idx.tolist())) == len(idx)
        assert np.all(allowed[i, idx])
        rest = allowed[i].copy()
        rest[idx] = False
        if rest.any():
            assert s64[i, rest].max() <= ref.min() + 2 * E[i], (i, s64[i, rest].max(), ref.min(), E[i])


def cos64(rows, q):
    return (q @ rows.T) / np.sqrt((rows * rows).sum(1))[None, :]


@pytest.mark.parametrize("D", [5, 32, 300])
def test_gaussian_rows_within_the_fp32_bound(lib, gpu, D):
    """E = 2 (D + 8) 2^-24 |q|: the worst case of a D-term fp32 fma chain (D 2^-24 sum |q_i r_i| <=
    D 2^-24 |q| |r|, Cauchy-Schwarz) divided by |r|, plus the roundings of r.r, sqrt and the
    division."""
    keys, rows, q = real_case(D)
    t = fill(lib, D, keys, rows, "v", "f32")
    rng = np.random.default_rng(4)
    excl = np.stack([rng.choice(keys, 2, replace=False) for _ in range(len(q))])
    cand = rng.choice(keys, 1200, replace=False)
    q64 = q.astype(np.float64)
    s64 = cos64(rows, q64)
    E = 2.0 * (D + 8) * 2.0 ** -24 * np.linalg.norm(q64, axis=1)
    everything = np.ones(s64.shape, dtype=bool)
    gk, gs = t.nearest(q, k=10, part="v", metric="cos")
    check_against_fp64(gk, gs, s64, keys, E, everything)
    allowed = np.isin(keys, cand)[None, :] & ~np.stack([np.isin(keys, e) for e in excl])
    gk, gs = t.nearest(q, k=10, part="v", metric="cos", exclude=excl, candidates=cand)
    check_against_fp64(gk, gs, s64, keys, E, allowed)
    t.close()


# ---- 4. analogy ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,metric", [(100, "f32", "cos"), (5, "f64", "dot")])
def test_analogy_integer_rows_bit_exact(lib, gpu, D, dtype, metric):
    from swiftmpi_amd.evaluate import topk_order
    keys, rows, _ = int_case(D, 1031, 1, seed=21)
    t = fill(lib, D, keys, rows, "v", dtype)
    rng = np.random.default_rng(6)
    ia = np.stack([rng.choice(len(keys), 3, replace=False) for _ in range(70)])
    abc = keys[ia]
    r32 = rows.astype(np.float32)
    q = (r32[ia[:, 1]] - r32[ia[:, 0]]) + r32[ia[:, 2]]
    wk, ws = topk_order(f32_scores(rows, q, metric), keys, 10, abc)
    gk, gs = t.analogy(abc, k=10, part="v", metric=metric)
    assert np.array_equal(gk, wk) and np.array_equal(gs, ws)
    dk, ds = as_np(*t.analogy(torch.as_tensor(abc.view(np.int64), device=gpu), k=10, part="v", metric=metric))
    assert np.array_equal(dk, wk) and np.array_equal(ds, ws)
    t.close()


@functools.lru_cache(maxsize=None)
def planted_case(D, seed=17, entities=40, relations=4, distractors=1500, nquest=500):
    """Rows E_i + R_j + N(0, 0.15) for 40 entities x 4 relations plus Gaussian distractors."""
    rng = np.random.default_rng(seed + D)
    ent, rel = rng.normal(0, 1, (entities, D)), rng.normal(0, 1, (relations, D))
    words = ["e%d_r%d" % (i, j) for i in range(entities) for j in range(relations)]
    rows = np.stack([ent[i] + rel[j] + rng.normal(0, 0.15, D) for i in range(entities) for j in range(relations)])
    words += ["d%d" % i for i in range(distractors)]
    rows = np.concatenate([rows, rng.normal(0, 1, (distractors, D))]).astype(np.float32).astype(np.float64)
    keys = make_keys(rng, len(words))
    quest = []
    while len(quest) < nquest:
        a, b = rng.choice(entities, 2, replace=False)
        x, y = rng.choice(relations, 2, replace=False)
        quest.append(("e%d_r%d" % (a, x), "e%d_r%d" % (a, y), "e%d_r%d" % (b, x), "e%d_r%d" % (b, y)))
    return words, keys, rows, quest


@pytest.mark.parametrize("D", [32, 300])
def test_analogy_planted_table(lib, gpu, D):
    from swiftmpi_amd.synth import analogy_accuracy_table
    words, keys, rows, quest = planted_case(D)
    key_of = dict(zip(words, (int(x) for x in keys))).__getitem__
    row_of = {w: i for i, w in enumerate(words)}
    t = fill(lib, D, keys, rows, "v", "f32")
    ia = np.array([[row_of[w] for w in qu[:3]] for qu in quest])
    abc = keys[ia]
    a, b, c = rows[ia[:, 0]], rows[ia[:, 1]], rows[ia[:, 2]]
    q64 = (b - a) + c
    s64 = cos64(rows, q64)
    # the query's own fp32 rounding: two additions of D-vectors, then through the scoring chain
    E = 2.0 * (D + 8) * 2.0 ** -24 * np.linalg.norm(q64, axis=1) + (D + 10) * 2.0 ** -24 * (
        np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1) + np.linalg.norm(c, axis=1))
    allowed = ~np.stack([np.isin(keys, e) for e in abc])
    gk, gs = t.analogy(abc, k=1, part="v", metric="cos")
    check_against_fp64(gk, gs, s64, keys, E, allowed)
    assert analogy_accuracy_table(t, quest, words, key_of) == 1.0
    t.close()


# ---- 5. errors ---------------------------------------------------------------------------------
def test_errors_leave_the_table_usable(lib, gpu):
    sw = lib
    keys, rows, q = int_case(32, 33, 2, seed=2)
    t = fill(sw, 32, keys, rows, "v", "f32")
    good = t.nearest(q, k=3)

    def code(fn):
        with pytest.raises(sw.SwpsError) as e:
            fn()
        return e.value.code

    cfg, badkey = -5, -2
    assert code(lambda: t.nearest(q, k=0)) == cfg
    assert code(lambda: t.nearest(q, k=65)) == cfg
    assert code(lambda: t.nearest(q, k=3, part=2)) == cfg
    assert code(lambda: t.nearest(q, k=3, metric=7)) == cfg
    assert code(lambda: t.nearest(q, k=3, exclude=np.zeros((2, 9), dtype=np.uint64))) == cfg
    assert code(lambda: t.analogy(keys[:3][None, :], k=0)) == cfg
    unknown = np.array([[keys[0], keys[1], np.uint64(12345)]], dtype=np.uint64)
    assert code(lambda: t.analogy(unknown, k=1)) == badkey
    lr = sw.Table("lr", capacity=64)
    assert code(lambda: sw.capi.check(sw.capi.lib().swps_nearest_h(
        lr.h, 0, 0, sw.capi.ptr(q), 1, 1, None, 0, None, 0, sw.capi.ptr(np.zeros(1, np.uint64)),
        sw.capi.ptr(np.zeros(1, np.float32))))) == cfg
    lr.close()
    ek, es = t.nearest(np.zeros((0, 32), dtype=np.float32), k=3)  # nq == 0
    assert ek.shape == (0, 3) and es.shape == (0, 3)
    again = t.nearest(q, k=3)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    ak, _ = t.analogy(keys[:3][None, :], k=2)
    assert not set(ak[0].tolist()) & set(keys[:3].tolist())
    t.close()


def test_most_similar_excludes_the_word(lib, gpu, tmp_path):
    from conftest import zipf_corpus
    sw = lib
    path = zipf_corpus(str(tmp_path / "c.txt"), 40, 60, seed=3)
    t = sw.Table("w2v", dim=16, capacity=200, dtype="f32", init="hash", seed=5)
    w = sw.Word2Vec(t, unigram_size=10 ** 5, init="table", minibatch=20)
    w.load_text(path)
    w.init()
    vk, _ = w.vocab()
    word = "w1"
    assert sw.bkdr(word) in set(int(x) for x in vk)
    got = w.most_similar(word, topn=5)
    many = w.most_similar([word, int(vk[3])], topn=5)
    assert got.shape == (5,) and many.shape == (2, 5) and np.array_equal(many[0], got)
    # by definition: Table.nearest of the word's own v row, the word excluded
    me = np.array([sw.bkdr(word)], dtype=np.uint64)
    v = t.export(torch.as_tensor(me.view(np.int64), device=gpu))[:, 16:32].cpu().numpy()
    wk, _ = t.nearest(v, k=5, part="v", metric="cos", exclude=me[None, :])
    assert np.array_equal(got, wk[0])
    assert sw.bkdr(word) not in got.tolist() and set(got.tolist()) <= set(int(x) for x in vk)
    top, _ = t.nearest(v, k=1, part="v", metric="cos")
    assert int(top[0, 0]) == sw.bkdr(word)  # unexcluded, a row's nearest row is itself
    w.close()
    t.close()


# ---- 6. routed tables --------------------------------------------------------------------------
def test_routed_world1_equals_local(lib, gpu):
    from swiftmpi_amd.comm import Comm
    comm = Comm.rccl(0, 1, port=_port())
    keys, rows, q = int_case(100, 1031, 33, seed=5)
    a, b = fill(lib, 100, keys, rows, "h", "f32"), fill(lib, 100, keys, rows, "h", "f32")
    a.route(comm, frag_num=1000)
    ak, as_ = a.nearest(q, k=64, part="h", metric="cos")
    bk, bs = b.nearest(q, k=64, part="h", metric="cos")
    assert np.array_equal(ak, bk) and np.array_equal(as_, bs)
    rng = np.random.default_rng(2)
    abc = keys[np.stack([rng.choice(len(keys), 3, replace=False) for _ in range(70)])]
    ak, as_ = a.analogy(abc, k=10, part="h")
    bk, bs = b.analogy(abc, k=10, part="h")
    assert np.array_equal(ak, bk) and np.array_equal(as_, bs)
    a.finish()
    a.close()
    b.close()
    comm.close()


def test_routed_two_ranks(lib, gpu):
    """Two gloo ranks on one GPU (tests/dist_nearest_check.py): both ranks' answers equal each
    other's and an unrouted table's, bit for bit."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()),
           os.path.join(ROOT, "tests", "dist_nearest_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-6000:])
    print("\n".join(ln for ln in r.stderr.splitlines() if "rank0" in ln or "Error" in ln)[-6000:])
    assert r.returncode == 0 and "NEAREST OK" in r.stdout


# ---- 7. non-finite scores: the order's NaN class, infinities, inf * 0, an overflowing r.r ---------
BIG = 1.5 * 2.0 ** 63  # 1.38e19, exact in fp32; BIG * BIG = 2.25 * 2^126 is finite, twice that is not
NF_ROWS, NF_NQ = 200, 35
NF_FIRST = 150  # the doctored rows: clear of int_case's duplicated rows (0..39) and its zero row (100)
NF_ZPOS = (1, 4)  # where query 0 holds zeros and the "inf0" row its infinities


@functools.lru_cache(maxsize=None)
def nonfinite_case(D):
    """int_case with a dozen doctored rows (name -> index in `names`) and three doctored queries:
    query 0 holds 0 at NF_ZPOS, query 33 a NaN, query 34 a +inf."""
    keys, rows, q = int_case(D, NF_ROWS, NF_NQ, seed=900 + D)
    nan, inf = np.nan, np.inf
    names = {}

    def put(name, values, fill=None):  # values: {position: value}; fill: the other elements (None: the integers)
        i = names[name] = NF_FIRST + len(names)
        if fill is not None:
            rows[i] = fill
        for p, v in values.items():
            rows[i, p] = v

    put("one_nan", {1: nan})
    put("tail_nan", {D - 1: nan})
    put("all_nan", {}, fill=nan)
    put("pinf", {0: inf})
    put("pinf_twin", {0: inf})
    rows[names["pinf_twin"]] = rows[names["pinf"]]  # equal infinite scores: the smaller key first
    put("ninf", {2: -inf})
    put("both_inf", {0: inf, 3: -inf})
    put("inf0", {p: inf for p in NF_ZPOS})
    put("all_pinf", {}, fill=inf)
    for name, vals in (("big_even_odd", {0: BIG, 3: BIG}), ("big_even", {0: BIG, 2: BIG}), ("big_mixed", {1: -BIG, 4: BIG})):
        put(name, vals, fill=0)
    q[0, list(NF_ZPOS)] = 0
    q[33, 2] = nan
    q[34, 0] = inf
    return keys, rows, q, names


def check_total_order(gk, gs):
    """The contract's order read off the answer alone: numbers (higher first, ties by smaller key),
    then NaN scores by ascending key, then the ~0 / -inf padding."""
    for i in range(gk.shape[0]):
        pad = gk[i] == EMPTY
        nan = np.isnan(gs[i]) & ~pad
        cls = np.where(pad, 2, np.where(nan, 1, 0))
        assert np.all(np.diff(cls) >= 0), (i, cls.tolist())
        assert np.all(np.isneginf(gs[i][pad]))
        nk = gk[i][nan]
        assert np.all(nk[1:] > nk[:-1]), (i, nk.tolist())
        num_s, num_k = gs[i][cls == 0], gk[i][cls == 0]
        assert np.all((num_s[1:] < num_s[:-1]) | ((num_s[1:] == num_s[:-1]) & (num_k[1:] > num_k[:-1]))), i


def check_scores(gk, gs, wk, ws, what):
    assert np.array_equal(gk, wk), what
    nan = np.isnan(ws)
    assert np.array_equal(np.isnan(gs), nan), what
    assert np.array_equal(gs[~nan], ws[~nan]), what


@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("D", [5, 32, 100])
def test_non_finite_scores(lib, gpu, monkeypatch, D, dtype, metric):
    """NaN and infinite values in rows and queries, which the suite's other query tests never hold.

    The reference, from IEEE 754 alone.  A score is the chain acc = fma(r[k], q[k], acc) over k from
    acc = 0 (the padded k tail adds fma(0, 0, acc) = acc), under cos divided by sqrt(r.r), r.r two such
    chains (even and odd k) added.  Every finite entry is a small integer, so as long as acc is finite
    it is exact, and
      - a NaN operand makes the product NaN and every later acc NaN;
      - inf * 0 is NaN (the "inf0" row against query 0; the +inf query against rows holding 0 there);
      - +inf and -inf terms in one chain: inf + -inf is NaN, whichever comes first ("both_inf" against
        a query whose elements there have one sign; of opposite signs the two terms are one infinity);
      - infinities of one sign only: that infinity ("pinf", "ninf", "all_pinf"), and equal infinite
        scores are a tie that the smaller key wins ("pinf_twin");
      - cos: r.r of a row with a NaN is NaN and s / NaN is NaN; with an infinity r.r = +inf, sqrt
        gives +inf, and an infinite dot / +inf is NaN while a finite one gives a signed zero, which
        compares equal to the zero row's 0 (a tie by key);
      - the "big" rows: BIG^2 = 2.25 * 2^126 is finite in fp32 and the second such term overflows to
        +inf, in one chain ("big_even") or at the final even + odd addition ("big_even_odd"); their
        dots (3 q_a +- 3 q_b) * 2^62 are exact (the other elements are 0), so cos gives +-0 and dot
        the largest finite scores of the table.
    The order of the additions never decides the CLASS of the result (NaN, +inf, -inf, finite), and
    the finite results are exact, so elementwise fp64 products summed in any order and rounded to
    fp32 once (f32_scores) are the chain's values; the NaN's sign and payload are not compared.
    r.r cast from fp64 overflows to +inf exactly where the fp32 chain does: all its terms are >= 0."""
    from swiftmpi_amd.evaluate import topk_order
    keys, rows, q, names = nonfinite_case(D)
    part = "v" if D != 32 else "h"
    t = fill(lib, D, keys, rows, part, dtype)
    ref = f32_scores(rows, q, metric)
    # the derivation above, spot-checked on the reference before it judges the kernel
    col = {n: ref[:, i] for n, i in names.items()}
    assert np.isnan(col["one_nan"]).all() and np.isnan(col["all_nan"]).all() and np.isnan(col["tail_nan"]).all()
    assert np.isnan(col["inf0"][0]) and np.isnan(ref[33]).sum() >= NF_ROWS - 1
    same = q[:33, 0] * q[:33, 3] >= 0  # inf * q0 and -inf * q3 of opposite signs (or an inf * 0)
    assert same.any() and not same.all()
    assert np.array_equal(np.isnan(col["both_inf"][:33]), same if metric == "dot" else np.ones(33, dtype=bool))
    if metric == "dot":
        fin = q[:33, 0] != 0
        assert np.array_equal(col["pinf"][:33][fin], np.where(q[:33, 0][fin] > 0, np.inf, -np.inf).astype(np.float32))
        assert np.array_equal(col["big_even_odd"][:33], ((3 * q[:33, 0] + 3 * q[:33, 3]) * 2.0 ** 62).astype(np.float32))
    else:
        assert np.isnan(col["pinf"][:33][q[:33, 0] != 0]).all()  # inf / inf
        assert not col["big_even"][:33].any() and not col["big_even_odd"][:33].any()  # finite / inf = +-0
        assert not ref[33, NF_ROWS // 2] and not np.isnan(ref[33, NF_ROWS // 2])  # the zero row under a NaN query
    rng = np.random.default_rng(D)
    nan_rows = keys[[names["one_nan"], names["all_nan"], names["tail_nan"], names["both_inf"]]]
    excl = np.stack([rng.choice(keys, 3) for _ in range(NF_NQ)])
    excl[:, 2] = EMPTY
    excl[::2, 0] = nan_rows[0]
    excl[1::3, 1] = nan_rows[3]
    # 40 candidates: every doctored row, plain rows, and keys the table lacks; k = 64 then lists the
    # numbers, the NaN scores and the padding of one query side by side
    cand = np.concatenate([keys[NF_FIRST:NF_FIRST + len(names)], rng.choice(keys[:NF_FIRST], 23, replace=False),
                           make_keys(rng, 5) + np.uint64(1)])
    twin = fill(lib, D, keys, rows, part, dtype, order=rng.permutation(len(keys)), capacity=777)
    seen_nan_before_pad = False
    for batch in (None, "32"):
        if batch:
            monkeypatch.setenv("SWPS_NEAREST_BATCH", batch)  # 35 queries: two batches
        for k in (1, 10, 64):
            for e, c in ((None, None), (excl, cand)):
                what = (D, dtype, metric, k, e is not None, batch)
                wk, ws = topk_order(ref, keys, k, e, c)
                gk, gs = t.nearest(q, k=k, part=part, metric=metric, exclude=e, candidates=c)
                check_scores(gk, gs, wk, ws, what)
                check_total_order(gk, gs)
                tk, ts = twin.nearest(q, k=k, part=part, metric=metric, exclude=e, candidates=c)
                assert np.array_equal(tk, gk) and np.array_equal(ts.view(np.uint32), gs.view(np.uint32)), what
                seen_nan_before_pad |= bool(((gk[:, :-1] != EMPTY) & np.isnan(gs[:, :-1]) & (gk[:, 1:] == EMPTY)).any())
    assert seen_nan_before_pad
    # the device form, and an analogy whose operand rows hold the non-finite values
    dk, ds = as_np(*t.nearest(torch.as_tensor(q, device=gpu), k=10, part=part, metric=metric))
    wk, ws = topk_order(ref, keys, 10)
    check_scores(dk, ds, wk, ws, "device")
    ia = np.stack([rng.choice(len(keys), 3, replace=False) for _ in range(NF_NQ)])
    nf = len(names) - 3  # not the "big" rows: BIG next to small integers in one query is not exact in fp32
    ia[:nf, 1] = np.arange(NF_FIRST, NF_FIRST + nf)
    ia[:nf, 0], ia[:nf, 2] = 3, 7
    r32 = rows.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        aq = (r32[ia[:, 1]] - r32[ia[:, 0]]) + r32[ia[:, 2]]
        wk, ws = topk_order(f32_scores(rows, aq, metric), keys, 10, keys[ia])
    gk, gs = t.analogy(keys[ia], k=10, part=part, metric=metric)
    check_scores(gk, gs, wk, ws, "analogy")
    check_total_order(gk, gs)
    tk, ts = twin.analogy(keys[ia], k=10, part=part, metric=metric)
    assert np.array_equal(tk, gk) and np.array_equal(ts.view(np.uint32), gs.view(np.uint32))
    t.close()
    twin.close()
