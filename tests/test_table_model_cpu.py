"""CPU guard for tests/test_table_model_gpu.py (no GPU): the NumPy model of the shard
(tests/table_model.py) and the inputs the GPU tests feed it can tell right from wrong.

  - the vectorised model equals a scalar restatement (Python floats, math.sqrt);
  - a doctored model differs from the true one in at least one element of EVERY hot row
    (a row pushed by two or more sources), on exactly the inputs of the GPU cases;
  - one element of one quarter off by one ulp fails the comparison helper.

What each doctoring can show depends on the table type, by arithmetic, not by choice of inputs:
  reverse   sources applied in reverse order: both dtypes (the step of a source divides by the
            sum that already holds the earlier sources' squares).
  noround   no rounding to T between sources: fp32 tables.  On an fp64 table T is the type of
            the arithmetic, the omitted rounding is the identity, and the doctored model must
            EQUAL the true one (asserted).
  reassoc   a * (lr / sqrt(..)) for (a * lr) / sqrt(..): fp64 W2V tables and LR tables (whose
            arithmetic is in T).  On an fp32 W2V table the two fp64 quotients differ by one
            fp64 ulp at most, which the cast of h + step to fp32 absorbs except about once in
            2^29 elements: no input of a few hundred rows can show it, and the GPU tests
            cannot see such a kernel change on fp32 tables either.
"""
import numpy as np
import pytest

import table_model as tm
from table_model import (LR_SERVED_N, LR_SINGLE_N, SERVED_DIMS, SERVED_N, SORT_LOGCAPS, WORLDS, context_accepts,
                         served_case, single_case)


def _apply(model, case):
    model.assign(case["keys"], case["rows"])
    for g in case["grads"]:
        model.push_sources(case["skeys"], g, case["counts"])
    return model.export(case["keys"])


def _model(case, doctor=None):
    return tm.TableModel(case["layout"], dim=case["D"], dtype=case["dtype"], learning_rate=case["lr"],
                         doctor=doctor)


W2V_CASES = [(dtype, gtype, D, world) for dtype, gtype in (("f32", "f32"), ("f32", "f64"), ("f64", "f64"))
             for D in SERVED_DIMS if context_accepts(dtype, D) for world in WORLDS]


@pytest.fixture(scope="module")
def truth():
    cache = {}

    def get(layout, dtype, gtype, D, world):
        key = (layout, dtype, gtype, D, world)
        if key not in cache:
            case = served_case(layout, dtype, gtype, D, world)
            cache[key] = (case, _apply(_model(case), case))
        return cache[key]
    return get


def _hot_index(case):
    hot = set(case["hot"].tolist())
    idx = np.array([i for i, k in enumerate(case["keys"].tolist()) if k in hot])
    assert len(idx) >= SERVED_N // 2  # two thirds of the keys are pushed by two or more sources
    return idx


def test_generator_shape():
    """The properties section 3 of the GPU module relies on."""
    for world in WORLDS:
        case = served_case("w2v", "f32", "f32", 8, world)
        counts = case["counts"].astype(int)
        off = np.concatenate([[0], np.cumsum(counts)])
        per = [case["skeys"][off[r]:off[r + 1]] for r in range(world)]
        assert all(len(set(p.tolist())) == len(p) for p in per)  # distinct within a source
        times = np.bincount(np.searchsorted(np.sort(case["keys"]), case["skeys"]), minlength=SERVED_N)
        live = int((counts > 0).sum())
        assert (times == 1).any() and (times == min(2, live)).any() and (times == live).any()
        assert (counts == 0).any() == (world == 5)
        assert times.max() >= 3 or world == 2  # runs of three or more sources on one row
        # opposite orders: the keys the first and the last non-empty source share
        a, b = per[0], [p for p in per if len(p)][-1]
        shared = set(a.tolist()) & set(b.tolist())
        assert len(shared) > 10
        assert [k for k in a.tolist() if k in shared] == [k for k in b.tolist() if k in shared][::-1]
        g = case["grads"][0]
        assert (g == 0).any() and (np.abs(g) > 50).any() and not (g[:, 0] == 0).any()
        assert (case["rows"][:, 2 * 8:] > 0).all()  # non-zero second-moment sums
    single = served_case("w2v", "f32", "f32", 8, 3, single=True)
    assert (single["counts"] > 0).sum() == 1 and len(single["hot"]) == 0


@pytest.mark.parametrize("dtype,gtype,D,world", [c for c in W2V_CASES if c[2] in (4, 8, 260, 300)])
@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
def test_vectorised_model_equals_scalar_restatement_w2v(dtype, gtype, D, world, rule):
    case = served_case("w2v", dtype, gtype, D, world)
    m = tm.TableModel("w2v", dim=D, dtype=dtype, learning_rate=case["lr"], rule=rule)
    got = _apply(m, case)
    off = np.concatenate([[0], np.cumsum(case["counts"].astype(int))])
    sample = list(range(0, SERVED_N, 11))[:6]
    for i in sample:
        key = case["keys"][i]
        per_push = []
        for g in case["grads"]:
            per_push += [g[j] for r in range(world) for j in range(off[r], off[r + 1]) if case["skeys"][j] == key]
        want = tm.scalar_w2v_row(case["rows"][i], per_push, m.lr, m.fudge, rule, tm.DT[dtype])
        assert tm.same_bits(got[i], want), (i, len(per_push))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
def test_vectorised_model_equals_scalar_restatement_lr(dtype, rule):
    case = served_case("lr", dtype, "f32", 1, 3, n=400)
    m = tm.TableModel("lr", dtype=dtype, learning_rate=case["lr"], rule=rule)
    got = _apply(m, case)
    for i in range(0, 400, 7):
        key = case["keys"][i]
        per_push = [g[j, 0] for g in case["grads"] for j in np.flatnonzero(case["skeys"] == key)]
        want = tm.scalar_lr_row(case["rows"][i], per_push, m.lr, m.fudge, rule, tm.DT[dtype])
        assert tm.same_bits(got[i], want), i


@pytest.mark.parametrize("dtype,gtype,D,world", W2V_CASES)
def test_doctored_w2v_models_differ_in_every_hot_row(truth, dtype, gtype, D, world):
    case, true = truth("w2v", dtype, gtype, D, world)
    hot = _hot_index(case)
    tb = tm.bits(true)
    for doctor in ("reverse", "noround", "reassoc"):
        bad = tm.bits(_apply(_model(case, doctor), case))
        if doctor == "noround" and dtype == "f64":
            assert np.array_equal(bad, tb)  # rounding fp64 to fp64: the identity
            continue
        if doctor == "reassoc" and dtype == "f32":
            continue  # absorbed by the cast to fp32 (module docstring)
        differs = (bad != tb).any(axis=1)
        assert differs[hot].all(), (doctor, int((~differs[hot]).sum()), len(hot))
        cold = np.setdiff1d(np.arange(len(tb)), hot)
        if doctor != "reassoc":  # order and rounding between sources only matter with two sources
            assert not differs[cold].any()


def _zero_share(g):
    return float((np.asarray(g) == 0).mean())


def test_lr_pushes_carry_zero_gradients():
    """Every LR push of the GPU module (single source, served, sort configurations) carries
    about 2 % exact zeros: gen_grads draws them with probability 0.02, and the smallest push
    has 1536 gradients (31 expected zeros, standard deviation 5.5)."""
    pushes = []
    for dtype in ("f32", "f64"):
        for rule in ("adagrad", "sgd"):
            pushes += [g for _, g in single_case("lr", 1, dtype, rule, LR_SINGLE_N, np.float32)["pushes"]]
    for world in WORLDS:
        pushes += served_case("lr", "f32", "f32", 1, world)["grads"]
    pushes += served_case("lr", "f32", "f32", 1, 3, single=True)["grads"]
    pushes += [tm.sort_case_grads(logcap) for logcap in SORT_LOGCAPS]
    assert len(pushes) == 20
    for g in pushes:
        assert g.dtype == np.float32 and g.shape[1] == 1 and len(g) >= 1536
        assert 0.005 < _zero_share(g) < 0.04, (len(g), _zero_share(g))
        assert (np.abs(g) > 50).any()
    # a zero gradient on a hot row of the served cases: the multi kernel meets m == 0 inside a run
    for world in WORLDS:
        case = served_case("lr", "f32", "f32", 1, world)
        hot = np.isin(case["skeys"], case["hot"])
        assert all((g[hot, 0] == 0).any() for g in case["grads"])


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_doctored_lr_models_differ(dtype, world):
    """An LR row holds one weight and one sum, so it cannot always show a difference, and the
    bar here is a share of rows, not `every hot row` (which is asked of W2V rows above): the
    doctored models must differ in the weight of more than half of the hot rows (reverse: the
    first step divides by another sum; a zero gradient among a row's sources, about one row
    in 20, can hide it) and of more than a tenth of all rows (reassoc: two roundings in T
    against two others, equal about half the time)."""
    case = served_case("lr", dtype, "f32", 1, world, n=LR_SERVED_N)
    true = tm.bits(_apply(_model(case), case))
    hot = set(case["hot"].tolist())
    idx = np.array([i for i, k in enumerate(case["keys"].tolist()) if k in hot])
    rev = tm.bits(_apply(_model(case, "reverse"), case))
    assert (rev[idx, 0] != true[idx, 0]).mean() > 0.5
    rea = tm.bits(_apply(_model(case, "reassoc"), case))
    assert (rea[:, 0] != true[:, 0]).mean() > 0.1


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_ulp_fails_the_comparison(dtype):
    case = served_case("w2v", dtype, dtype, 8, 3)
    true = _apply(_model(case), case)
    tm.assert_rows_equal(true.copy(), true)
    T = tm.DT[dtype]
    for quarter in range(4):
        for up in (True, False):
            bad = true.copy()
            r, e = 17 + quarter, quarter * 8 + 3
            bad[r, e] = np.nextafter(bad[r, e], T(np.inf if up else -np.inf), dtype=T)
            assert not tm.same_bits(bad, true)
            with pytest.raises(AssertionError, match=("h", "v", "h2", "v2")[quarter] + ": 1 of"):
                tm.assert_rows_equal(bad, true)
    neg = true.copy()
    neg[0, 0] = T(0.0)
    pos = neg.copy()
    neg[0, 0] = -neg[0, 0]
    with pytest.raises(AssertionError):  # -0.0 is not +0.0
        tm.assert_rows_equal(neg, pos)
    lr = np.array([[0.5, 1.0]], dtype=T)
    bad = lr.copy()
    bad[0, 1] = np.nextafter(bad[0, 1], T(2), dtype=T)
    with pytest.raises(AssertionError, match="g2: 1 of"):
        tm.assert_rows_equal(bad, lr, layout="lr")


def test_hash_init_model_is_the_written_definition():
    """hash_init against a scalar restatement with Python integers (mod 2^64)."""
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9e3779b97f4a7c15) & M
        x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & M
        x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & M
        return x ^ (x >> 31)

    def uh(seed, key, i):
        z = sm(seed ^ sm((key + 0x632be59bd9b4e019 * (i + 1)) & M))
        return np.float32(z >> 40) * np.float32(1.0 / 16777216.0)

    keys = np.array([0, 1, 2 ** 64 - 2, 0x123456789abcdef0], dtype=np.uint64)
    for seed in (0, 3, 2 ** 63 + 5):
        for T in (np.float32, np.float64):
            got = tm.hash_init(seed, keys, "w2v", 5, T)
            for r, k in enumerate(keys.tolist()):
                want = [T((float(uh(seed, k, e)) - 0.5) / 5.0) for e in range(10)] + [T(0)] * 10
                assert tm.same_bits(got[r], np.array(want, dtype=T))
            lr = tm.hash_init(seed, keys, "lr", 1, T)
            assert tm.same_bits(lr, np.array([[T(uh(seed, k, 0)), 0] for k in keys.tolist()], dtype=T))
    assert (np.abs(tm.hash_init(1, keys, "w2v", 5, np.float64)[:, :10]) <= 0.1).all()


def test_model_pull_inserts_hash_init_rows():
    """TableModel.pull on keys across the u64 range, repeated keys included."""
    keys = tm.gen_keys(np.random.default_rng(1), 50)
    assert keys.max() > 2 ** 63 and len(set(keys.tolist())) == 50
    m = tm.TableModel("w2v", dim=3, dtype="f32", seed=9)
    twice = np.concatenate([keys, keys[:5]])
    v = m.pull(twice)
    assert m.size() == 50 and tm.same_bits(v, tm.hash_init(9, twice, "w2v", 3, np.float32)[:, :6])
    assert tm.same_bits(m.export(keys), tm.hash_init(9, keys, "w2v", 3, np.float32))
    m.push(keys[:7], np.ones((7, 6)))
    assert tm.same_bits(m.pull(keys)[7:], v[7:50]) and not tm.same_bits(m.pull(keys)[:7], v[:7])
