"""Removing keys from the HBM shard (swps_erase, swps_prune, swps_table_shrink: swps_erase.hip and
the relaxed move of swps_table.hip).

The fixtures are tests/test_table_grow_gpu.py's: its 67 keys (0, 1, 2^64 - 2, a consecutive run,
keys over the u64 range) pulled 3, 5, 9, 17 and 33 at a time, W2V D = 8 and D = 300 and LR in f32
and f64.  The row order after an erase is compared with tests/erase_model.py applied to the order
read before it; rows are compared per key through export, bit for bit (same_bits)."""

import numpy as np
import pytest
import torch

import erase_model as em
import table_model as tm
from conftest import zipf_corpus

pytestmark = pytest.mark.gpu

SEED = 11
RATE = 0.7
E_OOM, E_BADKEY, E_CFG, E_STATE, E_UNSUPPORTED = -1, -2, -5, -6, -7
CEIL = 1024
KEYS = np.concatenate([np.array([0, 1, 2 ** 64 - 2], dtype=np.uint64), np.arange(1000, 1030, dtype=np.uint64),
                       tm.gen_keys(np.random.default_rng(1), 34)])
np.random.default_rng(2).shuffle(KEYS)
CHUNKS = np.split(KEYS, np.cumsum([3, 5, 9, 17]))
ABSENT = np.array([2, 999, 1030, 2 ** 63 + 12345, 2 ** 64 - 3], dtype=np.uint64)
PAD = np.array([2 ** 64 - 1], dtype=np.uint64)
CONFIGS = [("w2v", 8, "f32"), ("w2v", 8, "f64"), ("w2v", 300, "f32"), ("w2v", 300, "f64"), ("lr", 1, "f32"),
           ("lr", 1, "f64")]
CONFIG_IDS = ["%s-D%d-%s" % c for c in CONFIGS]
SOME = [CONFIGS[0], CONFIGS[3], CONFIGS[4], CONFIGS[5]]
SOME_IDS = [CONFIG_IDS[0], CONFIG_IDS[3], CONFIG_IDS[4], CONFIG_IDS[5]]


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).to("cuda")


def host(t):
    return t.cpu().numpy()


def create_slots(capacity):
    ns = 1
    while ns < 2 * capacity:
        ns <<= 1
    return ns


def code_of(exc):
    return exc.value.code


def make(lib, layout, D, dtype, init="hash", capacity=256, **kw):
    return lib.Table(layout, dim=D, dtype=dtype, learning_rate=RATE, init=init, seed=SEED, capacity=capacity, **kw)


def gtype(layout):
    return np.float64 if layout == "w2v" else np.float32


def nonzero_grads(rng, n, t, layout):
    g = tm.gen_grads(rng, n, t.push_elems, gtype(layout))
    g[g == 0] = 0.5  # every accumulator of a pushed row becomes positive
    return g


def filled(lib, layout, D, dtype, seed, **kw):
    """A table holding the 67 keys, each pushed once with a random gradient."""
    t = make(lib, layout, D, dtype, **kw)
    for c in CHUNKS:
        t.pull(dev(c))
    t.push(dev(KEYS), dev(tm.gen_grads(np.random.default_rng(seed), 67, t.push_elems, gtype(layout))))
    assert t.size() == 67
    return t


def find_h(lib, t, keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.zeros(len(keys), dtype=np.uint8)
    lib.capi.check(lib.capi.lib().swps_table_find_h(t.h, lib.capi.ptr(keys), len(keys), lib.capi.ptr(out)))
    return out


def erase_checked(lib, t, layout, gone, listed=None, on_host=False):
    """Erase `listed` (default: `gone`) and check the whole contract against the state before:
    the count, the size, the row order (erase_model), every survivor's row, the absence of `gone`."""
    gone = np.asarray(gone, dtype=np.uint64)
    listed = gone if listed is None else listed
    before = t.keys()
    rows = host(t.export(dev(before))) if len(before) else None
    cap = t.capacity()
    n = t.erase(listed if on_host else dev(listed))
    assert n == len(gone)
    assert t.size() == len(before) - len(gone)
    dead = np.isin(before, gone)
    assert int(dead.sum()) == len(gone)
    after = t.keys()
    assert np.array_equal(after, em.apply(before, dead)), "the row order is not the compaction rule's"
    if len(after):
        tm.assert_rows_equal(host(t.export(dev(after))), rows[[int(np.nonzero(before == k)[0][0]) for k in after]],
                             layout, "survivors")
        assert np.all(find_h(lib, t, after) == 1)
    if len(gone):
        assert np.all(find_h(lib, t, gone) == 0)
    assert t.capacity() == cap  # capacity, ceiling, slots and growths are untouched
    return after


def test_the_keys_are_the_growth_tests(lib):
    assert len(KEYS) == 67 and len(set(KEYS.tolist())) == 67 and [len(c) for c in CHUNKS] == [3, 5, 9, 17, 33]
    assert {0, 1, 2 ** 64 - 2} <= set(KEYS.tolist()) and not set(ABSENT.tolist()) & set(KEYS.tolist())


# ==== 1. the core contract, per config ============================================================
@pytest.mark.parametrize("layout,D,dtype", CONFIGS, ids=CONFIG_IDS)
def test_core_erase(lib, gpu, layout, D, dtype):
    t = filled(lib, layout, D, dtype, seed=3)
    rng = np.random.default_rng([4, D, dtype == "f64"])
    gone = rng.permutation(KEYS)[:20]
    listed = rng.permutation(np.concatenate([gone, ABSENT, PAD, gone[:6]]))  # 20 present, 5 absent, ~0, 6 repeats
    assert len(listed) == 32
    erase_checked(lib, t, layout, gone, listed)
    assert t.size() == 47
    v, found = t.lookup(dev(gone), insert=False, return_found=True)
    assert not host(found).any() and not host(v).any()
    assert t.size() == 47
    g = tm.gen_grads(rng, 1, t.push_elems, gtype(layout))
    with pytest.raises(lib.SwpsError) as e:
        t.push(dev(gone[:1]), dev(g))
    assert code_of(e) == E_BADKEY
    t.close()


# ==== 2. a removed key is a new key ================================================================
@pytest.mark.parametrize("init", ["hash", "zero"])
@pytest.mark.parametrize("layout,D,dtype", SOME, ids=SOME_IDS)
def test_fresh_init_on_repull(lib, gpu, layout, D, dtype, init):
    t = filled(lib, layout, D, dtype, seed=5, init=init)
    fresh = make(lib, layout, D, dtype, init=init)
    gone = np.random.default_rng(6).permutation(KEYS)[:12]
    erase_checked(lib, t, layout, gone)
    v, w = host(t.pull(dev(gone))), host(fresh.pull(dev(gone)))
    assert tm.same_bits(v, w), "a re-pull after an erase is not the pull of a new key"
    tm.assert_rows_equal(host(t.export(dev(gone))), host(fresh.export(dev(gone))), layout, "re-pulled")
    assert t.size() == 67
    t.close()
    fresh.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_flcg_draws_continue(lib, gpu, dtype):
    """The float-LCG draw state does not move with an erase: new keys after it take the draws they
    take on a twin that never erased, and a removed key that comes back takes the next draw."""
    t, twin = make(lib, "lr", 1, dtype, init="flcg"), make(lib, "lr", 1, dtype, init="flcg")
    a, b, c = KEYS[:30], KEYS[30:50], KEYS[50:60]
    assert tm.same_bits(host(t.pull(dev(a))), host(twin.pull(dev(a))))
    gone = a[[0, 3, 4, 9, 17, 20, 21, 22, 28, 29]]
    erase_checked(lib, t, "lr", gone)
    assert tm.same_bits(host(t.pull(dev(b))), host(twin.pull(dev(b))))
    # ten draws either way: the returning keys on t, ten other new keys on the twin
    assert tm.same_bits(host(t.pull(dev(gone))), host(twin.pull(dev(c))))
    assert t.size() == 50 and twin.size() == 60
    t.close()
    twin.close()


# ==== 3. the named masks ============================================================================
@pytest.mark.parametrize("layout,D,dtype", SOME, ids=SOME_IDS)
def test_named_masks(lib, gpu, layout, D, dtype):
    t = filled(lib, layout, D, dtype, seed=7)
    # nothing: an empty list (device and host), absent keys and padding only
    assert t.erase(dev(np.zeros(0, dtype=np.uint64))) == 0 and t.erase(np.zeros(0, dtype=np.uint64)) == 0
    order = t.keys()
    erase_checked(lib, t, layout, [], np.concatenate([ABSENT, PAD]))
    assert np.array_equal(t.keys(), order)
    # only the last rows: no row moves
    order = erase_checked(lib, t, layout, order[-9:])
    assert len(order) == 58
    # only the first rows: the last rows fill them, in ascending order
    first = order[:7]
    after = erase_checked(lib, t, layout, first, on_host=True)
    assert np.array_equal(after[:7], order[-7:]) and np.array_equal(after[7:], order[7:-7])
    t.close()
    # 60 of 67: more dead than survivors
    t = filled(lib, layout, D, dtype, seed=8)
    after = erase_checked(lib, t, layout, np.random.default_rng(9).permutation(KEYS)[:60])
    assert len(after) == 7
    # everything, then the keys come back as new keys
    erase_checked(lib, t, layout, after)
    assert t.size() == 0 and len(t.keys()) == 0
    assert t.erase(dev(KEYS)) == 0  # an empty shard
    fresh = make(lib, layout, D, dtype)
    assert tm.same_bits(host(t.pull(dev(KEYS))), host(fresh.pull(dev(KEYS))))
    assert t.size() == 67
    ks = np.sort(KEYS)
    tm.assert_rows_equal(host(t.export(dev(ks))), host(fresh.export(dev(ks))), layout, "refilled")
    t.close()
    fresh.close()


@pytest.mark.parametrize("layout,D,dtype,n", [("lr", 1, "f32", 5000), ("lr", 1, "f64", 1100), ("w2v", 300, "f32", 700),
                                              ("w2v", 5, "f64", 1500)],
                         ids=["lr-f32-5000", "lr-f64-1100", "w2v-D300-f32-700", "w2v-D5-f64-1500"])
def test_many_rows(lib, gpu, layout, D, dtype, n):
    """Several blocks of every kernel and a scan longer than one tile; rows of 8 B (the 4-B copy
    lanes), 16 B, 4800 B and 160 B."""
    rng = np.random.default_rng([10, n])
    keys = tm.gen_keys(rng, n)
    t = make(lib, layout, D, dtype, capacity=n + 3)
    t.assign(dev(keys), dev(tm.gen_rows(rng, n, layout, D, tm.DT[dtype])))
    assert t.size() == n
    for share in (0.4, 0.03):
        held = t.keys()
        erase_checked(lib, t, layout, rng.permutation(held)[:int(share * len(held))])
    t.close()


# ==== 4. the freed rows are reusable ===============================================================
@pytest.mark.parametrize("layout,D,dtype", [CONFIGS[0], CONFIGS[4]], ids=[CONFIG_IDS[0], CONFIG_IDS[4]])
def test_row_reuse(lib, gpu, layout, D, dtype):
    t, twin = make(lib, layout, D, dtype, capacity=8), make(lib, layout, D, dtype)
    t.pull(dev(KEYS[:8]))
    assert t.size() == 8
    erase_checked(lib, t, layout, KEYS[[1, 4, 6]])
    t.pull(dev(KEYS[8:11]))  # no SWPS_E_OOM: the three freed rows
    assert t.size() == 8
    with pytest.raises(lib.SwpsError) as e:
        t.pull(dev(KEYS[11:12]))  # a ninth key
    assert code_of(e) == E_OOM and t.size() == 8
    assert t.erase(dev(KEYS[8:9])) == 1  # also drops the slot the overflow claimed without a row
    assert t.size() == 7 and find_h(lib, t, KEYS[11:12])[0] == 0
    held = np.concatenate([KEYS[[0, 2, 3, 5, 7]], KEYS[9:12]])
    v = host(t.pull(dev(held)))  # KEYS[11] inserts now
    assert t.size() == 8 and set(t.keys().tolist()) == set(held.tolist())
    assert tm.same_bits(v, host(twin.pull(dev(held))))
    assert t.capacity() == dict(capacity=8, max_capacity=0, slots=16, growths=0)
    t.close()
    twin.close()


# ==== 5. an erased table is the table of its survivors =============================================
@pytest.mark.parametrize("layout,D,dtype", CONFIGS, ids=CONFIG_IDS)
def test_twin_of_the_survivors(lib, gpu, layout, D, dtype):
    rng = np.random.default_rng([12, D, dtype == "f64"])
    t = filled(lib, layout, D, dtype, seed=13)
    gone = rng.permutation(KEYS)[:25]
    live = erase_checked(lib, t, layout, gone)
    twin = make(lib, layout, D, dtype)
    twin.assign(dev(live), t.export(dev(live)))
    new = np.arange(5000, 5012, dtype=np.uint64)
    pulled = rng.permutation(np.concatenate([live[:20], gone[:10], new]))
    dup = rng.choice(np.concatenate([live, gone[:10], new]), 300)
    dup[::37] = PAD[0]
    G = np.float64 if layout == "w2v" else np.float32
    gdup = rng.normal(0, 0.3, (300, t.push_elems)).astype(G)
    off = np.array([0, 0, 5, 130, 131, 300], dtype=np.int64)
    out = []
    for x in (t, twin):
        r = [host(x.pull(dev(pulled)))]
        x.push(dev(pulled[:30]), dev(tm.gen_grads(np.random.default_rng(14), 30, x.push_elems, gtype(layout))))
        x.push_dup(dev(dup), dev(gdup), "mean", -1.0)
        r.append(host(x.lookup_bag(dev(dup), dev(off), mode="sum", insert=False)))
        out.append(r)
    for a, b in zip(*out):
        assert tm.same_bits(a, b)
    assert t.size() == twin.size() == 42 + 10 + 12
    ks = np.sort(t.keys())
    assert np.array_equal(ks, np.sort(twin.keys()))
    tm.assert_rows_equal(host(t.export(dev(ks))), host(twin.export(dev(ks))), layout, "twin")
    t.close()
    twin.close()


# ==== 6. queries, snapshots ==========================================================================
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_nearest_skips_erased_keys(lib, gpu, dtype):
    D, n = 12, 40
    rng = np.random.default_rng(15)
    keys = KEYS[:n]
    rows = np.zeros((n, 4 * D))
    rows[:, :2 * D] = rng.integers(-4, 5, (n, 2 * D))
    rows[:, 2 * D:] = 7.0
    t = make(lib, "w2v", D, dtype, init="zero")
    t.assign(dev(keys), dev(rows.astype(tm.DT[dtype])))
    order = t.keys()
    targets = np.array([order[0], order[n // 2], order[-1]])  # a hole a mover fills, a middle row, the last row
    q = np.stack([rows[int(np.nonzero(keys == k)[0][0]), D:2 * D] for k in targets]).astype(np.float32)
    k6, s6 = t.nearest(q, k=6, part="v", metric="cos")
    assert np.array_equal(k6[:, 0], targets), "a row is not its own nearest neighbour"
    erase_checked(lib, t, "w2v", targets)
    k2, s2 = t.nearest(q, k=2, part="v", metric="cos")
    for i in range(3):  # the answer before, without the erased keys: the next candidates move up
        keep = ~np.isin(k6[i], targets)
        assert np.array_equal(k2[i], k6[i][keep][:2]) and tm.same_bits(s2[i], s6[i][keep][:2])
    abc = np.array([[targets[0], order[1], order[2]]], dtype=np.uint64)
    with pytest.raises(lib.SwpsError) as e:
        t.analogy(abc, k=1)
    assert code_of(e) == E_BADKEY
    ka, _ = t.analogy(np.array([[order[1], order[2], order[3]]], dtype=np.uint64), k=5)
    assert not set(ka.reshape(-1).tolist()) & set(targets.tolist())
    t.close()


def test_snapshot_of_an_erased_table(lib, gpu, tmp_path):
    t = filled(lib, "w2v", 8, "f32", seed=16)
    live = erase_checked(lib, t, "w2v", np.random.default_rng(17).permutation(KEYS)[:30])
    path = str(tmp_path / "t.snap")
    t.save(path)
    u = make(lib, "w2v", 8, "f32", init="zero", capacity=40)
    u.restore(path)
    assert u.size() == 37 and set(u.keys().tolist()) == set(live.tolist())
    tm.assert_rows_equal(host(u.export(dev(live))), host(t.export(dev(live))), "w2v", "restored")
    # and back into the erased table itself, after more erases: the file's keys return
    erase_checked(lib, t, "w2v", live[:5])
    t.restore(path)
    assert t.size() == 37
    tm.assert_rows_equal(host(t.export(dev(live))), host(u.export(dev(live))), "w2v", "restored in place")
    t.close()
    u.close()


# ==== 7. pinning =====================================================================================
def test_pinned_tables_refuse(lib, gpu, tmp_path):
    path = zipf_corpus(str(tmp_path / "c.txt"), 40, 60, seed=21)
    t = lib.Table("w2v", dim=16, dtype="f32", init="hash", seed=7, capacity=200)
    w = lib.Word2Vec(t, window=3, negative=4, minibatch=20, sample=1e-3, unigram_size=10 ** 6, init="table")
    w.load_text(path)
    w.init()
    V = t.size()
    held = t.keys()
    for call in (lambda: t.erase(dev(held[:3])), lambda: t.erase(held[:3]), lambda: t.prune(0.0), lambda: t.shrink(),
                 lambda: t.erase(dev(np.zeros(0, dtype=np.uint64)))):
        with pytest.raises(lib.SwpsError) as e:
            call()
        assert code_of(e) == E_STATE
    assert t.size() == V and np.array_equal(t.keys(), held) and t.capacity()["capacity"] == 200
    w.train(1)
    w.close()
    erase_checked(lib, t, "w2v", held[:3])
    t.prune(0.0)
    t.shrink()
    assert t.capacity()["capacity"] == max(t.size(), 1)
    t.close()


# ==== 8. prune =======================================================================================
PRUNE_CONFIGS = CONFIGS + [("w2v", 7, "f32")]  # D odd: the accumulator half is not 16-B aligned in fp32
PRUNE_IDS = CONFIG_IDS + ["w2v-D7-f32"]


def acc_max(rows, layout):
    """Per row the largest accumulator element, as the table dtype holds it."""
    half = rows.shape[1] // 2
    return rows[:, half:].max(axis=1)


@pytest.mark.parametrize("layout,D,dtype", PRUNE_CONFIGS, ids=PRUNE_IDS)
def test_prune(lib, gpu, layout, D, dtype):
    rng = np.random.default_rng([18, D, dtype == "f64"])
    t = make(lib, layout, D, dtype)
    keys = KEYS[:40]
    t.pull(dev(keys))
    hot = rng.permutation(keys)[:15]
    t.push(dev(hot), dev(nonzero_grads(rng, 15, t, layout)))
    order = t.keys()
    rows = host(t.export(dev(order)))
    assert t.prune(0.0) == 25  # the keys that never received a gradient
    dead = ~np.isin(order, hot)
    assert np.array_equal(t.keys(), em.apply(order, dead))
    after = t.keys()
    tm.assert_rows_equal(host(t.export(dev(after))), rows[[int(np.nonzero(order == k)[0][0]) for k in after]], layout,
                         "kept")
    assert t.prune(0.0) == 0 and t.size() == 15
    # a threshold strictly between two accumulator maxima, from the rows as they are
    order = t.keys()
    rows = host(t.export(dev(order)))
    mx = acc_max(rows, layout).astype(np.float64)
    s = np.sort(mx)
    assert s[6] < s[7]
    thr = float(s[6]) + (float(s[7]) - float(s[6])) / 2
    assert s[6] < thr < s[7]
    cold = mx <= thr
    assert int(cold.sum()) == 7
    assert t.prune(thr) == 7
    assert np.array_equal(t.keys(), em.apply(order, cold))
    # exactly at a maximum: <= keeps nothing of that row
    order = t.keys()
    mx = acc_max(host(t.export(dev(order))), layout).astype(np.float64)
    assert t.prune(float(np.sort(mx)[0])) == int((mx <= np.sort(mx)[0]).sum())
    # a NaN accumulator element is never cold
    nan_key = np.array([777], dtype=np.uint64)
    row = np.zeros((1, t.row_elems), dtype=tm.DT[dtype])
    row[0, -1] = np.nan
    t.assign(dev(nan_key), dev(row))
    n = t.size()
    assert t.prune(1e300) == n - 1
    assert t.keys().tolist() == [777]
    t.close()


@pytest.mark.parametrize("D,dtype", [(300, "f32"), (7, "f32"), (8, "f64"), (67, "f64")])
def test_prune_sees_every_accumulator_element(lib, gpu, D, dtype):
    """Row j has one positive accumulator element, at position j of [h2sum | v2sum], and large h and
    v; four more rows are all-zero accumulators.  prune(0) removes the four."""
    n = 2 * D
    rows = np.zeros((n + 4, 4 * D), dtype=tm.DT[dtype])
    rows[:, :2 * D] = 9.0  # h and v are not accumulators
    rows[np.arange(n), 2 * D + np.arange(n)] = np.finfo(tm.DT[dtype]).tiny
    keys = tm.gen_keys(np.random.default_rng(19), n + 4)
    t = make(lib, "w2v", D, dtype, init="zero", capacity=n + 4)
    t.assign(dev(keys), dev(rows))
    assert t.prune(0.0) == 4
    assert set(t.keys().tolist()) == set(keys[:n].tolist())
    assert t.prune(float(np.finfo(tm.DT[dtype]).tiny)) == n
    t.close()


def test_prune_needs_the_accumulators(lib, gpu):
    t = make(lib, "w2v", 8, "f32", push_rule="sgd")
    t.pull(dev(KEYS[:5]))
    with pytest.raises(lib.SwpsError) as e:
        t.prune(0.0)
    assert code_of(e) == E_UNSUPPORTED and t.size() == 5
    assert t.erase(dev(KEYS[:2])) == 2  # erase does not read them
    t.close()


# ==== 9. shrink ======================================================================================
@pytest.mark.parametrize("layout,D,dtype", SOME, ids=SOME_IDS)
def test_shrink(lib, gpu, layout, D, dtype):
    t = make(lib, layout, D, dtype, capacity=4, max_capacity=CEIL)
    for c in CHUNKS:
        t.pull(dev(c))
    t.push(dev(KEYS), dev(tm.gen_grads(np.random.default_rng(20), 67, t.push_elems, gtype(layout))))
    t.reserve(150)
    c0 = t.capacity()
    assert c0["capacity"] >= 128 and t.size() == 67
    live = erase_checked(lib, t, layout, np.random.default_rng(21).permutation(KEYS)[:57])
    assert len(live) == 10
    rows = host(t.export(dev(live)))
    t.shrink()
    assert t.capacity() == dict(capacity=10, max_capacity=CEIL, slots=create_slots(10), growths=c0["growths"] + 1)
    assert t.size() == 10 and np.array_equal(t.keys(), live)  # a move keeps the row indices
    tm.assert_rows_equal(host(t.export(dev(live))), rows, layout, "shrunk")
    t.shrink(1000)  # not below the capacity: nothing happens
    t.shrink(10)
    t.shrink(3)  # below the rows held: the rows held
    assert t.capacity()["capacity"] == 10 and t.capacity()["growths"] == c0["growths"] + 1
    # the ceiling still holds: the table grows again from the new count
    twin = make(lib, layout, D, dtype)
    new = np.arange(7000, 7020, dtype=np.uint64)
    assert tm.same_bits(host(t.pull(dev(new))), host(twin.pull(dev(new))))
    assert t.size() == 30 and 30 <= t.capacity()["capacity"] <= CEIL and t.capacity()["max_capacity"] == CEIL
    tm.assert_rows_equal(host(t.export(dev(live))), rows, layout, "regrown")
    t.reserve(100)
    g = t.capacity()["growths"]
    t.shrink(50)
    assert t.capacity() == dict(capacity=50, max_capacity=CEIL, slots=128, growths=g + 1) and t.size() == 30
    tm.assert_rows_equal(host(t.export(dev(live))), rows, layout, "shrunk again")
    t.close()
    twin.close()
    # an empty table shrinks to one row
    t = make(lib, layout, D, dtype, capacity=64)
    t.shrink()
    assert t.capacity() == dict(capacity=1, max_capacity=0, slots=2, growths=1) and t.size() == 0
    t.close()
