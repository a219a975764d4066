"""Growing the HBM shard (swps_table_reserve, swps_table_set_max_capacity, the move: k_rehash and
the row migration of swps_table.hip).

Every table here starts at capacity 4 (or 8) so that 40 to 70 keys force three or four moves.
The reference of every comparison is a twin table created large (capacity 256) and driven by the
identical call sequence, plus tests/table_model.py's TableModel where arithmetic is involved.
Comparisons are per key, through export / pull of a key list, and bit for bit (same_bits); row
indices are not compared (k_find_or_insert hands them out in atomic order)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import table_model as tm
from conftest import GOLDEN, free_port, word_dump, zipf_corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
RATE = 0.7
E_OOM, E_CFG, E_STATE = -1, -5, -6
CEIL = 1024
# 67 distinct keys: the extremes, a run of consecutive integers (neighbours under the small
# masks) and keys spread over the u64 range; pulled 3, 5, 9, 17 and 33 at a time
KEYS = np.concatenate([np.array([0, 1, 2 ** 64 - 2], dtype=np.uint64), np.arange(1000, 1030, dtype=np.uint64),
                       tm.gen_keys(np.random.default_rng(1), 34)])
np.random.default_rng(2).shuffle(KEYS)
CHUNKS = np.split(KEYS, np.cumsum([3, 5, 9, 17]))
CONFIGS = [("w2v", 8, "f32"), ("w2v", 8, "f64"), ("w2v", 300, "f32"), ("w2v", 300, "f64"), ("lr", 1, "f32"),
           ("lr", 1, "f64")]
CONFIG_IDS = ["%s-D%d-%s" % c for c in CONFIGS]


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


def pair(lib, layout, D, dtype, init="hash", capacity=4, ceiling=CEIL, **kw):
    """(the table under test, its twin created large)."""
    kw = dict(dim=D, dtype=dtype, learning_rate=RATE, init=init, seed=SEED, **kw)
    return (lib.Table(layout, capacity=capacity, max_capacity=ceiling, **kw), lib.Table(layout, capacity=256, **kw))


def code_of(exc):
    return exc.value.code


def check_shape(t, nkeys, min_growths):
    c = t.capacity()
    assert t.size() == nkeys
    assert c["growths"] >= min_growths and c["capacity"] >= nkeys, c
    assert c["slots"] == create_slots(c["capacity"]), c
    return c


def test_the_keys_are_what_the_docstring_says():
    assert len(KEYS) == 67 and len(set(KEYS.tolist())) == 67 and [len(c) for c in CHUNKS] == [3, 5, 9, 17, 33]
    assert {0, 1, 2 ** 64 - 2} <= set(KEYS.tolist()) and 2 ** 64 - 1 not in set(KEYS.tolist())


# ==== 1. pulls grow the table ====================================================================
@pytest.mark.parametrize("layout,D,dtype,init", [pytest.param(*c, i, id="%s-%s" % (cid, i))
                                                 for c, cid in zip(CONFIGS, CONFIG_IDS)
                                                 for i in ("hash", "zero", "flcg") if i != "flcg" or c[0] == "lr"])
def test_pull_growth(lib, gpu, layout, D, dtype, init):
    t, twin = pair(lib, layout, D, dtype, init)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=RATE, seed=SEED)
    assert t.capacity() == dict(capacity=4, max_capacity=CEIL, slots=8, growths=0)
    rng = np.random.default_rng(3)
    seen = np.zeros(0, dtype=np.uint64)
    for c in CHUNKS:
        # new keys; every call lists its keys in the same order on both tables (the flcg draws)
        v, w = host(t.pull(dev(c))), host(twin.pull(dev(c)))
        assert tm.same_bits(v, w), "a pull of new keys differs from the twin's"
        if init == "hash":
            assert tm.same_bits(v, m.pull(c))
        seen = np.concatenate([seen, c])
        old = rng.permutation(seen)[:max(2, len(seen) // 3)]  # keys held since earlier capacities
        assert tm.same_bits(host(t.pull(dev(old))), host(twin.pull(dev(old)))), "a re-pull differs"
        assert t.size() == len(seen)
    check_shape(t, 67, 3)
    assert twin.capacity()["growths"] == 0
    assert set(t.keys().tolist()) == set(KEYS.tolist())
    ks = np.sort(KEYS)
    tm.assert_rows_equal(host(t.export(dev(ks))), host(twin.export(dev(ks))), layout, "grown")
    t.close()
    twin.close()


# ==== 2. pushes between the growths ================================================================
def drive_pushes(t, twin, m, layout, rng, finish=False):
    G = np.float64 if layout == "w2v" else np.float32
    seen = np.zeros(0, dtype=np.uint64)
    for c in CHUNKS:
        v = host(t.pull(dev(c)))
        assert tm.same_bits(v, host(twin.pull(dev(c)))) and tm.same_bits(v, m.pull(c))
        seen = np.concatenate([seen, c])
        for _ in range(2):  # rows moved by earlier growths take further steps
            sub = rng.permutation(seen)[:max(2, (3 * len(seen)) // 4)]
            g = tm.gen_grads(rng, len(sub), m.P, G)
            for x in (t, twin):
                x.push(dev(sub), dev(g))
            m.push(sub, g)
    if finish:
        t.barrier()
        t.finish()
    ks = np.sort(KEYS)
    out = host(t.export(dev(ks)))
    tm.assert_rows_equal(out, host(twin.export(dev(ks))), layout, "twin")
    tm.assert_rows_equal(out, m.export(ks), layout, "model")
    check_shape(t, 67, 3)


@pytest.mark.parametrize("layout,D,dtype", CONFIGS, ids=CONFIG_IDS)
def test_push_across_growths(lib, gpu, layout, D, dtype):
    t, twin = pair(lib, layout, D, dtype)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=RATE, seed=SEED)
    drive_pushes(t, twin, m, layout, np.random.default_rng([4, D, dtype == "f64"]))
    t.close()
    twin.close()


@pytest.fixture(scope="module")
def comm1(lib, gpu):
    from swiftmpi_amd.comm import Comm
    comm = Comm.rccl(0, 1, port=free_port())
    yield comm
    comm.close()


# ==== 9a. a routed growable table at world 1 (and the multi-source push forms) ======================
@pytest.mark.parametrize("distinct", ["1", "0"])
@pytest.mark.parametrize("layout,D,dtype", CONFIGS, ids=CONFIG_IDS)
def test_routed_world1_growth(lib, gpu, comm1, monkeypatch, layout, D, dtype, distinct):
    """The owner side of a routed pull inserts through table_find_or_insert: the shard grows under
    the routed rounds.  SWPS_PUSH_DISTINCT=0 sends every push through k_push_keys, the sort and
    k_push_w2v_multi / k_push_lr_multi (table_push_sources' multi-source forms) on the moved rows."""
    monkeypatch.setenv("SWPS_PUSH_DISTINCT", distinct)
    t, twin = pair(lib, layout, D, dtype)
    t.route(comm1, frag_num=1000)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=RATE, seed=SEED)
    drive_pushes(t, twin, m, layout, np.random.default_rng([5, D, dtype == "f64"]), finish=True)
    t.close()
    twin.close()


# ==== 3. reserve ====================================================================================
@pytest.mark.parametrize("layout,D,dtype", CONFIGS, ids=CONFIG_IDS)
def test_reserve(lib, gpu, layout, D, dtype):
    t, twin = pair(lib, layout, D, dtype, ceiling=None)
    assert t.capacity()["max_capacity"] == 0
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=RATE, seed=SEED)
    first, rest = KEYS[:4], KEYS[4:64]
    G = np.float64 if layout == "w2v" else np.float32
    g = tm.gen_grads(np.random.default_rng(6), 4, m.P, G)
    for x in (t, twin):
        x.pull(dev(first))
        x.push(dev(first), dev(g))  # non-zero sums in the rows that move
    before, kb = host(t.export(dev(first))), t.keys()
    t.reserve(100)
    assert t.capacity() == dict(capacity=100, max_capacity=0, slots=256, growths=1)
    assert t.size() == 4 and np.array_equal(t.keys(), kb)  # row r still holds key r
    tm.assert_rows_equal(host(t.export(dev(first))), before, layout, "reserved")
    tm.assert_rows_equal(before, host(twin.export(dev(first))), layout, "twin")
    assert tm.same_bits(host(t.pull(dev(rest))), host(twin.pull(dev(rest))))
    assert t.size() == 64
    ks = np.sort(KEYS[:64])
    tm.assert_rows_equal(host(t.export(dev(ks))), host(twin.export(dev(ks))), layout, "after reserve")
    for n in (0, 4, 99, 100):  # already there: nothing moves
        t.reserve(n)
    assert t.capacity()["growths"] == 1 and t.capacity()["capacity"] == 100
    for n in (2 ** 32, 0xFFFFFFF0):
        with pytest.raises(lib.SwpsError) as e:
            t.reserve(n)
        assert code_of(e) == E_CFG
    assert t.capacity()["capacity"] == 100 and t.size() == 64
    t.close()
    twin.close()


# ==== 4. reserve repairs a table that overflowed ===================================================
@pytest.mark.parametrize("layout,D,dtype", [CONFIGS[0], CONFIGS[3], CONFIGS[4]],
                         ids=[CONFIG_IDS[0], CONFIG_IDS[3], CONFIG_IDS[4]])
def test_repair_after_overflow(lib, gpu, layout, D, dtype):
    t, twin = pair(lib, layout, D, dtype, capacity=8, ceiling=None)
    k12 = dev(KEYS[:12])
    with pytest.raises(lib.SwpsError) as e:  # the fixed-capacity contract
        t.pull(k12)
    assert code_of(e) == E_OOM
    assert t.size() == 8
    t.reserve(32)
    assert t.capacity()["capacity"] == 32
    v = host(t.pull(k12))  # the four keys that lost their slots insert again
    assert t.size() == 12
    assert tm.same_bits(v, host(twin.pull(k12)))
    assert set(t.keys().tolist()) == set(KEYS[:12].tolist())
    tm.assert_rows_equal(host(t.export(k12)), host(twin.export(k12)), layout, "repaired")
    t.close()
    twin.close()


# ==== 5. exact fit, the ceiling ====================================================================
def test_exact_fit_and_ceiling(lib, gpu):
    t, twin = pair(lib, "w2v", 8, "f32", capacity=8, ceiling=8)
    assert tm.same_bits(host(t.pull(dev(KEYS[:8]))), host(twin.pull(dev(KEYS[:8]))))
    assert t.capacity() == dict(capacity=8, max_capacity=8, slots=16, growths=0) and t.size() == 8
    with pytest.raises(lib.SwpsError) as e:
        t.pull(dev(KEYS[8:9]))
    assert code_of(e) == E_OOM and t.capacity()["growths"] == 0
    assert tm.same_bits(host(t.pull(dev(KEYS[:8]))), host(twin.pull(dev(KEYS[:8]))))  # held keys still pull
    t.close()
    t = lib.Table("w2v", dim=8, capacity=8, max_capacity=16, init="hash", seed=SEED)
    with pytest.raises(lib.SwpsError) as e:
        t.pull(dev(KEYS[:20]))
    assert code_of(e) == E_OOM
    assert t.capacity()["capacity"] == 16 and t.size() == 16
    for bad in (4, 15, 0xFFFFFFF0, 2 ** 40):  # below the capacity (16 now), out of range
        with pytest.raises(lib.SwpsError) as e:
            t.set_max_capacity(bad)
        assert code_of(e) == E_CFG
    assert t.capacity()["max_capacity"] == 16
    t.set_max_capacity(0)  # cleared: fixed at 16
    with pytest.raises(lib.SwpsError) as e:
        t.pull(dev(KEYS[20:24]))
    assert code_of(e) == E_OOM and t.capacity()["capacity"] == 16
    # raised: the slots the overflows spoiled are dropped by the next move and every key pulls
    t.set_max_capacity(64)
    assert tm.same_bits(host(t.pull(dev(KEYS[:24]))), host(twin.pull(dev(KEYS[:24]))))
    assert t.size() == 24 and 24 <= t.capacity()["capacity"] <= 64
    t.close()
    twin.close()


# ==== 6. the async forms and the host bound ========================================================
def test_async_bound(lib, gpu):
    from swiftmpi_amd import capi
    D = 8
    t, twin = pair(lib, "w2v", D, "f32")
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    k3 = dev(KEYS[:3])
    outs = [torch.empty((3, 2 * D), dtype=torch.float32, device="cuda") for _ in range(10)]
    torch.cuda.synchronize()
    for o in outs:  # the same three keys: n counts them ten times, the real count stays 3
        capi.check(capi.lib().swps_pull_async(t.h, capi.ptr(k3), 3, capi.ptr(o), sp))
    capi.check(capi.lib().swps_table_sync(t.h))
    assert t.size() == 3 and t.capacity()["capacity"] <= 8
    want3 = twin.pull(k3)
    for o in outs:
        assert torch.equal(o, want3)
    new = KEYS[3:53]
    parts = [dev(p) for p in np.split(new, [7, 20, 21])]  # 7, 13, 1 and 29 keys: growths between async calls
    outs = [torch.empty((p.numel(), 2 * D), dtype=torch.float32, device="cuda") for p in parts]
    torch.cuda.synchronize()
    for p, o in zip(parts, outs):
        capi.check(capi.lib().swps_pull_async(t.h, capi.ptr(p), p.numel(), capi.ptr(o), sp))
    capi.check(capi.lib().swps_table_sync(t.h))  # no error latched
    assert t.size() == 53
    for p, o in zip(parts, outs):
        assert torch.equal(o, twin.pull(p))
    check_shape(t, 53, 3)
    assert torch.equal(t.export(dev(np.sort(KEYS[:53]))), twin.export(dev(np.sort(KEYS[:53]))))
    t.close()
    twin.close()


# ==== 7. snapshots and dumps =======================================================================
def test_snapshot_into_a_small_table(lib, gpu, tmp_path):
    D = 8
    src = lib.Table("w2v", dim=D, capacity=256, learning_rate=RATE, init="hash", seed=SEED)
    k60 = np.sort(KEYS[:60])
    src.pull(dev(k60))
    src.push(dev(k60), dev(tm.gen_grads(np.random.default_rng(7), 60, 2 * D, np.float64)))
    snap = str(tmp_path / "t.snap")
    src.save(snap)
    rows = host(src.export(dev(k60)))
    t = lib.Table("w2v", dim=D, capacity=4, max_capacity=CEIL, learning_rate=RATE, init="zero")
    t.restore(snap)
    check_shape(t, 60, 1)
    assert set(t.keys().tolist()) == set(k60.tolist())
    tm.assert_rows_equal(host(t.export(dev(k60))), rows, "w2v", "restored")
    t.close()
    t = lib.Table("w2v", dim=D, capacity=4, max_capacity=32, learning_rate=RATE, init="zero")
    with pytest.raises(lib.SwpsError) as e:  # the file does not fit under the ceiling
        t.restore(snap)
    assert code_of(e) == E_OOM and t.capacity()["growths"] == 0 and t.size() == 0
    t.close()
    t = lib.Table("w2v", dim=D, capacity=4, learning_rate=RATE, init="zero")
    with pytest.raises(lib.SwpsError) as e:  # fixed capacity: as before
        t.restore(snap)
    assert code_of(e) == E_OOM and t.capacity() == dict(capacity=4, max_capacity=0, slots=8, growths=0)
    t.close()
    src.close()
    # the reference's text dump into a growable table
    dump = word_dump(str(tmp_path / "w.txt"), 50, D, seed=8)
    t = lib.Table("w2v", dim=D, capacity=4, max_capacity=CEIL)
    big = lib.Table("w2v", dim=D, capacity=256)
    t.load(dump)
    big.load(dump)
    check_shape(t, 50, 1)
    k50 = np.arange(1, 51, dtype=np.uint64)
    assert set(t.keys().tolist()) == set(k50.tolist())
    tm.assert_rows_equal(host(t.export(dev(k50))), host(big.export(dev(k50))), "w2v", "loaded")
    t.close()
    big.close()


# ==== 8. queries on a grown table ===================================================================
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_queries_after_growth(lib, gpu, dtype):
    D = 20
    rng = np.random.default_rng(9)
    rows = np.zeros((67, 4 * D))
    rows[:, :2 * D] = rng.normal(0, 1, (67, 2 * D)).astype(np.float32)
    rows[:, 2 * D:] = 7.0
    rows = rows.astype(tm.DT[dtype])
    t, twin = pair(lib, "w2v", D, dtype, init="zero")
    off = 0
    for c in CHUNKS:  # whole rows assigned 3, 5, 9, 17, 33 at a time: the table moves between them
        for x in (t, twin):
            x.assign(dev(c), dev(rows[off:off + len(c)]))
        off += len(c)
    check_shape(t, 67, 3)
    q = rng.normal(0, 1, (9, D)).astype(np.float32)
    abc = KEYS[np.stack([rng.choice(67, 3, replace=False) for _ in range(9)])]
    for part in ("v", "h"):
        (gk, gs), (ak, as_) = t.nearest(q, k=5, part=part, metric="cos"), t.analogy(abc, k=5, part=part)
        (wk, ws), (bk, bs) = twin.nearest(q, k=5, part=part, metric="cos"), twin.analogy(abc, k=5, part=part)
        assert gk.shape == (9, 5) and np.array_equal(gk, wk) and np.array_equal(ak, bk)
        assert gs.dtype == np.float32 and tm.same_bits(gs, ws) and tm.same_bits(as_, bs)
    t.close()
    twin.close()


# ==== 9b. two ranks, both shards growing ============================================================
def test_routed_two_ranks_grow(lib, gpu):
    """tests/dist_grow_check.py: two gloo ranks on one GPU, both shards from capacity 4, three rounds
    of overlapping pulls and pushes, against one unrouted table replaying the same sequence."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "dist_grow_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-6000:])
    print("\n".join(ln for ln in r.stderr.splitlines() if "rank0" in ln or "Error" in ln)[-6000:])
    assert r.returncode == 0 and "GROW OK" in r.stdout


# ==== 10. the app contexts =========================================================================
def test_word2vec_on_a_growable_table(lib, gpu, tmp_path):
    """init's full pull grows the table once to the vocabulary; from then on the context pins it
    and every step runs on fixed pointers: two epochs equal a table created large, bit for bit."""
    path = zipf_corpus(str(tmp_path / "c.txt"), 40, 60, seed=21)
    kw = dict(window=3, negative=4, minibatch=20, sample=1e-3, unigram_size=10 ** 6, init="table")
    out = []
    for tk in (dict(capacity=4, max_capacity=CEIL), dict(capacity=200)):
        t = lib.Table("w2v", dim=16, dtype="f32", init="hash", seed=7, **tk)
        w = lib.Word2Vec(t, **kw)
        w.load_text(path)
        V = w.info()["vocab"]
        assert 4 < V <= 60
        w.init()
        if "max_capacity" in tk:
            c = t.capacity()
            assert c["growths"] == 1 and c["capacity"] == V and t.size() == V
            with pytest.raises(lib.SwpsError) as e:
                t.reserve(10 ** 4)
            assert code_of(e) == E_STATE
            with pytest.raises(lib.SwpsError) as e:  # pinned: a new key past the capacity does not grow it
                t.pull(dev(np.array([2 ** 40 + 5], dtype=np.uint64)))
            assert code_of(e) == E_OOM and t.capacity()["capacity"] == V
        w.train(2)
        out.append((w.get_params(), w.stats()["lstate"]))
        w.close()
        if "max_capacity" in tk:
            t.reserve(10 ** 4)  # unpinned by the destroy
            assert t.capacity()["capacity"] == 10 ** 4 and t.size() == V
        t.close()
    (pa, la), (pb, lb) = out
    assert la == lb and tm.same_bits(pa, pb)


@pytest.mark.parametrize("plan,fast", [("step", False), ("none", True)])
def test_lr_on_a_growable_table(lib, gpu, plan, fast):
    data = os.path.join(GOLDEN, "lr_data.txt")
    out = []
    for tk in (dict(capacity=4, max_capacity=1 << 16), dict(capacity=4096)):
        t = lib.Table("lr", dtype="f32", learning_rate=0.05, **tk)
        m = lib.LR(t, minibatch=200, plan=plan, fast_sums=fast)
        m.load_text(data)
        V = m.info()["keys"]
        m.init()
        if "max_capacity" in tk:
            c = t.capacity()
            assert c["growths"] == 1 and c["capacity"] == V and t.size() == V
            with pytest.raises(lib.SwpsError) as e:
                t.reserve(10 ** 4)
            assert code_of(e) == E_STATE
        err = m.train(2)
        out.append((m.params(), err))
        m.close()
        if "max_capacity" in tk:
            t.reserve(10 ** 4)
            assert t.capacity()["capacity"] == 10 ** 4 and t.size() == V
        t.close()
    ((ka, wa, ga), ea), ((kb, wb, gb), eb) = out
    assert np.array_equal(ka, kb) and tm.same_bits(wa, wb) and tm.same_bits(ga, gb) and tm.same_bits(ea, eb)


def test_sent2vec_keeps_the_fixed_capacity(lib, gpu, tmp_path):
    """A sent2vec context pins its word table from its creation (its pass inserts pull misses while
    training kernels read the table): the known gap of DESIGN.md section 8.  The dump's 120 words
    grow the table to exactly 120 rows before the context exists; the corpus' other words then find
    no room, ceiling or not."""
    from conftest import int_corpus
    D = 16
    corpus = int_corpus(str(tmp_path / "c.txt"), 130, 150, seed=5)
    dump = word_dump(str(tmp_path / "w.txt"), 120, D, seed=6)
    words = {int(x) for line in open(corpus) for x in line.split()}
    assert len(words - set(range(1, 121))) > 0
    t = lib.Table("w2v", dim=D, capacity=4, max_capacity=CEIL, dtype="f64")
    s = lib.Sent2Vec(t, window=3, negative=4, minibatch=20, niters=1, unigram_size=10 ** 6)
    s.load_word_vector(dump)  # no context yet: the load grows the table
    assert t.capacity()["capacity"] == 120 and t.size() == 120
    with pytest.raises(lib.SwpsError) as e:
        s.load_text(corpus)
        s.train()
    assert code_of(e) == E_OOM and t.capacity()["capacity"] == 120
    with pytest.raises(lib.SwpsError) as e:
        t.reserve(500)
    assert code_of(e) == E_STATE
    s.close()
    t.reserve(500)
    assert t.capacity()["capacity"] == 500
    t.close()
