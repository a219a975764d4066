"""The sequence generator and the composed model of tests/shard_model.py, without a GPU: every
sequence the GPU test replays reaches what it is meant to reach, ShardModel gives what each
component model gives on that model's own cases, and every planted defect fails the same
step-by-step comparison the GPU test runs (swps_grow_plan is a host function of libswps)."""
import functools
import json

import numpy as np
import pytest

import admit_model as am
import bag_model as bm
import dup_model as dm
import erase_model as em
import shard_model as sm
import table_model as tm

U64 = np.uint64
CASES = sm.cases()
IDS = ["%s-seed%d" % (sm.cfg_id(c), s) for c, s in CASES]


@pytest.fixture(scope="module")
def plan(lib):
    return lib.grow_plan


@functools.lru_cache(maxsize=None)
def _sequence(cfg, seed, plan):
    return sm.gen_sequence(seed, cfg, plan=plan, with_model=True)


def _args_equal(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return type(a) is type(b) and a == b


def test_a_sequence_is_a_function_of_its_arguments(plan):
    cfg, seed = CASES[4]
    a, b = sm.gen_sequence(seed, cfg, plan=plan), sm.gen_sequence(seed, cfg, plan=plan)
    assert len(a) == len(b) == sm.STEPS
    for (op, x), (op2, y) in zip(a, b):
        assert op == op2 and sorted(x) == sorted(y) and all(_args_equal(x[k], y[k]) for k in x)
    c = sm.gen_sequence(seed + 100, cfg, plan=plan)
    assert [op for op, _ in c] != [op for op, _ in a]


def test_the_key_pool_is_small_and_holds_the_extremes():
    pool = set(sm.key_pool().tolist())
    assert len(pool) == 600 and {0, 1, 2 ** 64 - 2} <= pool and 2 ** 64 - 1 not in pool
    assert set(range(1000, 1030)) <= pool


@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_sequence_reaches_what_it_is_meant_to(plan, cfg, seed):
    """Every operation at least 3 times and in each of its forms (shard_model.VARIANTS; the forms of
    RARE_VARIANTS at least once), 3 growths, a shrink that moves, erases that move rows and
    erases that move none, calls that remove nothing, a key re-inserted into a reused row, an id
    refused and admitted later, one admitted within a call, an early admission at width 64, every
    call size after a strictly larger call among the repeated-key calls (they share one scratch) and,
    for lookup and push_dup, after a strictly larger call of the same operation, at most one expected error in twenty steps,
    a table that ends non-empty."""
    seq, model = _sequence(cfg, seed, plan)
    cov = sm.coverage(seq, model.events)
    print(sm.cfg_id(cfg), "seed", seed, json.dumps(cov, sort_keys=True))
    assert len(seq) == sm.STEPS
    assert sm.coverage_gaps(cov) == []
    # call sizes come from the stated set, and the table never passes 512 rows by more than a reserve
    for op, args in seq:
        if op in sm.DUP_KIND and op != "lookup_pad_err":
            assert len(args["keys"]) in sm.SIZES, (op, len(args["keys"]))
    assert cov["most_rows"] <= sm.CEIL + 16
    # after an overflow the very next step is the repair
    for i, (op, _) in enumerate(seq[:-1]):
        if op == "pull_oom":
            assert seq[i + 1][0] in ("erase", "erase_h", "reserve")


# ---- the composition gives what its parts give ------------------------------------------------------
def big(cfg, plan):
    return sm.ShardModel(cfg, capacity=1 << 14, max_capacity=0, plan=plan)


@pytest.mark.parametrize("layout,D,dtype,gtype,rule,reduce,scale", [("lr", 1, "f32", "f32", "adagrad", "mean", -1.0),
                                                                     ("w2v", 3, "f64", "f32", "adagrad", "sum", 1.0),
                                                                     ("w2v", 3, "f32", "f64", "sgd", "mean", 1.0)])
def test_agrees_with_dup_model(plan, layout, D, dtype, gtype, rule, reduce, scale):
    case = dm.push_case(layout, D, dtype, gtype)
    m = big((layout, D, dtype, rule, "zero"), plan)
    m.apply("assign", dict(keys=case["keys"], rows=case["rows"]))
    for k, g in case["calls"]:
        assert m.apply("push_dup", dict(keys=k, grads=g, reduce=reduce, scale=scale)) == {}
    assert tm.same_bits(m.export(case["keys"]), dm.run_case(case, rule, reduce, scale))


@pytest.mark.parametrize("layout,D,dtype", [("lr", 1, "f32"), ("w2v", 3, "f64")])
def test_agrees_with_bag_model(plan, layout, D, dtype):
    case = bm.bag_case(layout, D, dtype)
    for mode, weighted in (("sum", False), ("mean", False), ("sum", True)):
        m = big((layout, D, dtype, "adagrad", "hash"), plan)
        m.apply("assign", dict(keys=case["keys"], rows=case["rows"]))
        w = case["weights"] if weighted else None
        got = m.apply("lookup_bag", dict(keys=case["ids"], offsets=case["offsets"], weights=w, mode=mode, insert=True))
        assert tm.same_bits(got["out"], bm.forward(case, mode, weighted))
        gtype = "f64" if layout == "w2v" else "f32"
        for G in bm.bag_grads(case, gtype):
            assert m.apply("push_bag", dict(keys=case["ids"], offsets=case["offsets"], grads=G, weights=w, mode=mode)) == {}
        assert tm.same_bits(m.export(case["keys"]), bm.backward(case, gtype, "adagrad", mode, weighted))


@pytest.mark.parametrize("nu,min_count,width", [(255, 2, 64), (257, 5, 1 << 16)])
def test_agrees_with_admit_model(plan, nu, min_count, width):
    case = am.stream_case(nu, min_count)
    _, trace = am.run_stream(case, min_count, width)
    m = big(("lr", 1, "f32", "adagrad", "hash"), plan)
    m.apply("set_admission", dict(min_count=min_count, width=width))
    rows = 0
    for ids, want in zip(case["calls"], trace):
        assert m.apply("lookup_pad_err", dict(keys=ids)) == dict(error=sm.E_BADKEY)  # the calls hold ~0 padding
        got = m.apply("lookup", dict(keys=ids, insert=False, found=True))
        assert tm.same_bits(got["vals"], want["vals"]) and np.array_equal(got["found"], want["found"])
        assert np.array_equal(m.admission_cells(), want["cells"])
        assert {k: m.admission()[k] for k in want["counters"]} == want["counters"]
        assert np.array_equal(m.keys()[rows:], want["admitted"]) and m.loose == len(want["admitted"])
        rows = m.size()


def test_agrees_with_erase_model(plan):
    rng = np.random.default_rng(3)
    keys = tm.gen_keys(rng, 300)
    m = big(("w2v", 3, "f32", "adagrad", "hash"), plan)
    m.apply("pull", dict(keys=keys))
    for share in (0.0, 0.1, 0.5, 1.0):
        order = m.keys()
        dead = rng.random(len(order)) < share
        rows = m.export(order[~dead]) if (~dead).any() else None
        got = m.apply("erase", dict(keys=rng.permutation(np.concatenate([order[dead], order[dead][:5]]))))
        assert got == dict(n=int(dead.sum()))
        assert np.array_equal(m.keys(), em.apply(order, dead)) and m.size() == int((~dead).sum())
        if rows is not None:
            assert tm.same_bits(m.export(order[~dead]), rows)
        m.apply("pull", dict(keys=tm.gen_keys(rng, 40)))


# ---- every planted defect fails the comparison the GPU test runs -------------------------------------
@pytest.mark.parametrize("doctor", sm.DOCTORS)
def test_planted_defect_is_caught(plan, doctor):
    caught = []
    for (cfg, seed), name in zip(CASES, IDS):
        seq, _ = _sequence(cfg, seed, plan)
        # rows after every step, so that the step named is the one that did the damage
        bad = sm.replay(seq, sm.ShardModel(cfg, plan=plan), sm.ShardModel(cfg, plan=plan, doctor=doctor), name, every=1)
        if bad:
            caught.append((name,) + bad)
            print("%s: first failing step %d (%s) of %s: %s" % (doctor, bad[0], bad[1], name, bad[2]))
            if len(caught) == 2:
                break
    assert caught, "no chosen sequence tells the %r defect from the straight model" % doctor


class Shuffling(sm.ShardModel):
    """A straight model that uses the freedom a real table has: the new keys of one inserting call
    take their rows in a random order, and past the ceiling a random subset of them gets the rows."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.shuffle = np.random.default_rng(8)

    def _insert_call(self, new, bound, allow_oom=False):
        return super()._insert_call([new[i] for i in self.shuffle.permutation(len(new))], bound, allow_oom)


@pytest.mark.parametrize("cfg,seed", CASES, ids=IDS)
def test_replay_allows_what_the_table_leaves_undefined(plan, cfg, seed):
    """Row order inside one inserting call and the winners of an overflow are not defined: the
    comparison adopts them, and the sequence (drawn on a model that chose otherwise) still means the
    same: no accidental overflow, the same sizes, the same rows."""
    seq, _ = _sequence(cfg, seed, plan)
    other = Shuffling(cfg, plan=plan)
    assert sm.replay(seq, sm.ShardModel(cfg, plan=plan), other, "shuffling") is None
    assert any("error" in e and e["op"] == "pull_oom" for e in other.events)


@pytest.mark.parametrize("cfg,seed", CASES[::3], ids=IDS[::3])
def test_straight_model_replays_clean(plan, cfg, seed):
    """The comparison itself raises nothing on two straight models (and adopting an order is stable)."""
    seq, _ = _sequence(cfg, seed, plan)
    assert sm.replay(seq, sm.ShardModel(cfg, plan=plan), sm.ShardModel(cfg, plan=plan), "straight") is None
