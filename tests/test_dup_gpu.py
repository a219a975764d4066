"""The repeated-key calls of the HBM table (swiftmpi_amd/csrc/swps_dup.hip: swps_coalesce,
swps_lookup, swps_push_dup, their host forms and swiftmpi_amd.nn.SparseEmbedding) against the
NumPy model of tests/dup_model.py.  Every comparison is bit equality; tests/test_dup_cpu.py shows
on the CPU that the model and the inputs used here tell a wrong summation order from the right one.

Dispatch, as read from the source:
  gather      one thread per position (LR), 16-B lanes (row and pull bytes multiples of 16: f32
              even D, every f64 W2V table), scalar lanes (f32 odd D); D = 100 is one loop trip of
              the 64 lanes at f32, D = 300 has a tail trip
  reduce      lanes hold E = 16 / sizeof(G) gradient elements when 2 D % E == 0, else 1 (f32
              gradients at odd D); runs of <= 128 in one wave, longer runs as (run, chunk) items
"""
import numpy as np
import pytest
import torch

import dup_model as dm
import table_model as tm

pytestmark = pytest.mark.gpu

SEED = 11
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).to("cuda")


def host(t):
    return t.cpu().numpy()


def u64(t):
    return host(t).view(np.uint64)


def mk(lib, layout, D, dtype, rule="adagrad", capacity=4096, init="hash", **kw):
    return lib.Table(layout, dim=D, capacity=capacity, dtype=dtype, learning_rate=tm.LR_RATE, init=init, seed=SEED,
                     push_rule=rule, **kw)


# ==== coalesce ======================================================================================
def check_coalesce(t, keys):
    uniq, inv, count = t.coalesce(dev(keys))
    wu, wi, wc = dm.coalesce(keys)
    assert np.array_equal(u64(uniq), wu)
    assert np.array_equal(host(inv).astype(np.uint32), wi)  # -1 is 0xFFFFFFFF
    assert np.array_equal(host(count), wc.astype(np.int64))
    return wu


def test_coalesce(lib, gpu):
    t = mk(lib, "lr", 1, "f32", capacity=16)
    rng = np.random.default_rng(1)
    pool = tm.gen_keys(rng, 300)
    keys = pool[rng.integers(0, 300, 5000)]
    keys[rng.integers(0, 5000, 40)] = PAD
    wu = check_coalesce(t, keys)
    # the same as np.unique reordered by first index
    u, first, c = np.unique(keys[keys != PAD], return_index=True, return_counts=True)
    assert np.array_equal(wu, u[np.argsort(first)])
    check_coalesce(t, keys[:1])
    check_coalesce(t, np.full(777, pool[5]))
    check_coalesce(t, pool)
    check_coalesce(t, rng.permutation(np.concatenate([pool, pool[:7]])))
    check_coalesce(t, np.full(3, PAD))
    check_coalesce(t, np.array([PAD, pool[0], PAD, pool[0]]))
    assert t.size() == 0  # no row was touched
    shaped = t.coalesce(dev(keys[:60]).view(3, 20))[1]
    assert shaped.shape == (3, 20)
    t.close()


# ==== lookup ========================================================================================
LOOKUP_CASES = [("w2v", D, dt) for D in (4, 5, 6, 100, 300) for dt in ("f32", "f64")] + \
               [("lr", 1, "f32"), ("lr", 1, "f64")]


@pytest.mark.parametrize("layout,D,dtype", LOOKUP_CASES)
def test_lookup_inserts_each_new_key_once(lib, gpu, layout, D, dtype):
    rng = np.random.default_rng([2, D])
    t = mk(lib, layout, D, dtype)
    pool = tm.gen_keys(rng, 150)
    t.pull(dev(pool[:50]))  # some keys are there already
    keys = pool[rng.integers(0, 150, 2000)]
    nu = len(np.unique(keys))
    grew = len(np.setdiff1d(keys, pool[:50]))
    vals, found = t.lookup(dev(keys), insert=True, return_found=True)
    assert t.size() == 50 + grew and nu > grew
    P = t.pull_elems
    want = tm.hash_init(SEED, keys, layout, D, tm.DT[dtype])[:, :P]
    assert tm.same_bits(host(vals), want)
    assert host(found).all()
    # any shape; a second lookup inserts nothing and returns the same rows
    again = t.lookup(dev(keys).view(40, 50))
    assert again.shape == (40, 50, P) and torch.equal(again.view(2000, P), vals)
    assert t.size() == 50 + grew
    # the host form returns the wire type
    vh, fh = t.lookup(keys, return_found=True)
    wire = np.float64 if layout == "w2v" else np.float32
    assert tm.same_bits(vh, want.astype(wire)) and fh.all()
    t.close()


def test_lookup_flcg_draws_in_first_occurrence_order(lib, gpu):
    rng = np.random.default_rng(3)
    pool = tm.gen_keys(rng, 400)
    keys = pool[rng.integers(0, 400, 3000)]
    uniq, inv, _ = dm.coalesce(keys)
    a = mk(lib, "lr", 1, "f32", init="flcg")
    b = mk(lib, "lr", 1, "f32", init="flcg")
    got = host(a.lookup(dev(keys)))
    want = host(b.pull(dev(uniq)))
    assert len(np.unique(want)) > 300  # draws, not one value
    assert tm.same_bits(got, want[inv])
    # the draw state moved by the distinct count: the next new keys draw alike
    more = tm.gen_keys(np.random.default_rng(4), 10) ^ np.uint64(1 << 40)
    assert tm.same_bits(host(a.lookup(dev(np.repeat(more, 3)))), host(b.pull(dev(more)))[np.repeat(np.arange(10), 3)])
    a.close()
    b.close()


def test_lookup_without_insert(lib, gpu):
    rng = np.random.default_rng(5)
    t = mk(lib, "w2v", 6, "f32")
    pool = tm.gen_keys(rng, 60)
    t.pull(dev(pool[:30]))
    keys = pool[rng.integers(0, 60, 500)]
    keys[::17] = PAD
    vals, found = t.lookup(dev(keys), insert=False, return_found=True)
    there = np.isin(keys, pool[:30])
    assert np.array_equal(host(found).astype(bool), there) and there.any() and not there.all()
    want = tm.hash_init(SEED, keys, "w2v", 6, np.float32)[:, :12]
    want[~there] = 0
    assert tm.same_bits(host(vals), want)
    assert t.size() == 30
    t.barrier()  # nothing was latched
    # an inserting lookup refuses the empty key as swps_pull does
    with pytest.raises(lib.SwpsError) as e:
        t.lookup(dev(keys), insert=True)
    assert e.value.code == -2
    t.close()


def test_lookup_growth_counts_distinct_keys(lib, gpu):
    t = mk(lib, "w2v", 4, "f32", capacity=4, max_capacity=1 << 16)
    keys = np.tile(np.array([5, 6, 7], dtype=np.uint64), 1000)
    vals = t.lookup(dev(keys))
    assert t.size() == 3
    cap = t.capacity()
    assert cap["capacity"] <= max(4, 2 * 4, 0 + 3), cap  # n = 3000 would have grown it to 3000
    assert tm.same_bits(host(vals), tm.hash_init(SEED, keys, "w2v", 4, np.float32)[:, :8])
    t.close()


# ==== push_dup ======================================================================================
FULL = [(dt, gt, red, sc, rule) for dt in ("f32", "f64") for gt in ("f32", "f64") for red in ("sum", "mean")
        for sc in (1.0, -1.0) for rule in ("adagrad", "sgd")]
SOME = [(dt, gt, red, sc, rule) for dt in ("f32", "f64") for gt in ("f32", "f64")
        for red, sc, rule in (("sum", 1.0, "adagrad"), ("mean", -1.0, "sgd"))]
PUSH_CASES = [("w2v", D) + c for D in (4, 6, 300) for c in FULL] + [("w2v", 5) + c for c in SOME] + \
             [("lr", 1) + c for c in FULL if c[1] == "f32"]


@pytest.mark.parametrize("layout,D,dtype,gtype,reduce,scale,rule", PUSH_CASES)
def test_push_dup_equals_model(lib, gpu, layout, D, dtype, gtype, reduce, scale, rule):
    """Run lengths 1, 2, 3, 127, 128, 129, 257, 385 and 3000 with interleaved positions, two calls
    chained (the accumulators matter)."""
    case = dm.push_case(layout, D, dtype, gtype)
    t = mk(lib, layout, D, dtype, rule)
    dk = dev(case["keys"])
    t.assign(dk, dev(case["rows"]))
    for k, g in case["calls"]:
        t.push_dup(dev(k), dev(g), reduce, scale)
    want = dm.run_case(case, rule, reduce, scale)
    tm.assert_rows_equal(host(t.export(dk)), want, layout, "push_dup")
    t.close()


@pytest.mark.parametrize("layout,D,dtype", [("w2v", 6, "f32"), ("w2v", 5, "f64"), ("w2v", 300, "f32"),
                                            ("lr", 1, "f32")])
def test_push_dup_distinct_unknown_padding_host(lib, gpu, layout, D, dtype):
    rng = np.random.default_rng([6, D])
    n = 200
    keys = tm.gen_keys(rng, n)
    rows = tm.gen_rows(rng, n, layout, D, tm.DT[dtype])
    wire = np.float64 if layout == "w2v" else np.float32
    P = 2 * D if layout == "w2v" else 1
    a, b, c = (mk(lib, layout, D, dtype) for _ in range(3))
    dk = dev(keys)
    for t in (a, b, c):
        t.assign(dk, dev(rows))
    # distinct keys, scale 1: the table of swps_push
    g = tm.gen_grads(rng, n, P, wire)
    a.push_dup(dk, dev(g))
    b.push(dk, dev(g))
    c.push_dup(keys, g)  # the host form
    assert torch.equal(a.export(dk), b.export(dk))
    assert torch.equal(c.export(dk), b.export(dk))
    # repeats, padding and an unknown key: SWPS_E_BADKEY, the other keys applied
    m = tm.TableModel(layout, D, dtype, tm.LR_RATE)
    m.assign(keys, host(b.export(dk)))
    k2 = keys[rng.integers(0, 20, 600)]
    k2[::50] = PAD
    k2[7] = k2[300] = np.uint64(424242)
    g2 = tm.gen_grads(rng, 600, P, wire)
    for t, args in ((a, (dev(k2), dev(g2))), (c, (k2, g2))):
        with pytest.raises(lib.SwpsError) as e:
            t.push_dup(*args, reduce="mean", scale=0.5)
        assert e.value.code == -2
    assert dm.push_dup(m, k2, g2, "mean", 0.5).tolist() == [424242]
    tm.assert_rows_equal(host(a.export(dk)), m.export(keys), layout, "device form")
    tm.assert_rows_equal(host(c.export(dk)), m.export(keys), layout, "host form")
    assert a.size() == n
    for t in (a, b, c):
        t.close()


@pytest.mark.parametrize("gtype", ["f32", "f64"])
def test_push_dup_gradients_off_16_bytes(lib, gpu, gtype):
    """A contiguous gradient tensor that starts 4 (8) bytes into its storage takes the scalar
    lanes: the same table as the 16-B form."""
    case = dm.push_case("w2v", 6, "f32", gtype)
    a, b = mk(lib, "w2v", 6, "f32"), mk(lib, "w2v", 6, "f32")
    dk = dev(case["keys"])
    for t in (a, b):
        t.assign(dk, dev(case["rows"]))
    k, g = case["calls"][0]
    g = dev(g)
    base = torch.empty(g.numel() + 1, dtype=g.dtype, device="cuda")
    off = base[1:].view(g.shape)
    off.copy_(g)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0 and g.data_ptr() % 16 == 0
    a.push_dup(dev(k), g, "mean", -1.0)
    b.push_dup(dev(k), off, "mean", -1.0)
    assert torch.equal(a.export(dk), b.export(dk))
    a.close()
    b.close()


def test_push_dup_refuses_bad_arguments(lib, gpu):
    t = mk(lib, "lr", 1, "f32")
    k = dev(np.array([1, 1], dtype=np.uint64))
    t.lookup(k)
    with pytest.raises(lib.SwpsError) as e:
        t.push_dup(k, torch.zeros(2, 1, dtype=torch.float64, device="cuda"))
    assert e.value.code == -5  # an LR table takes fp32 gradients
    with pytest.raises(ValueError):
        t.push_dup(k, torch.zeros(2, 1, device="cuda"), reduce="max")
    t.push_dup(k[:0], torch.zeros(0, 1, device="cuda"))  # n = 0
    t.close()


# ==== routed, world 1 ===============================================================================
@pytest.mark.parametrize("layout,dtype", [("w2v", "f32"), ("w2v", "f64"), ("lr", "f32")])
def test_rccl_world1_routed_dup_equals_local(lib, gpu, layout, dtype):
    from conftest import free_port
    from swiftmpi_amd.comm import Comm
    D = 6 if layout == "w2v" else 1
    comm = Comm.rccl(0, 1, port=free_port())
    a, b = mk(lib, layout, D, dtype), mk(lib, layout, D, dtype)
    a.route(comm, frag_num=1000)
    rng = np.random.default_rng(7)
    pool = tm.gen_keys(rng, 120)
    for r in range(3):
        lens = rng.permutation(np.array([1, 2, 3, 130, 300] + [4] * 115))
        k = rng.permutation(np.repeat(pool, lens))
        k[::97] = PAD
        ka = dev(k[k != PAD])
        assert torch.equal(a.lookup(ka), b.lookup(ka))
        g = tm.gen_grads(rng, len(k), a.push_elems, np.float32 if r % 2 or layout == "lr" else np.float64)
        red = ("sum", "mean")[r % 2]
        a.push_dup(dev(k), dev(g), red, -1.0)
        b.push_dup(dev(k), dev(g), red, -1.0)
    a.push_dup(dev(k[:0]), dev(g[:0]))  # n = 0 still joins the exchange
    a.barrier()
    a.finish()
    assert a.route_stats()["rounds"] == 7
    keys = np.sort(b.keys())
    assert np.array_equal(np.sort(a.keys()), keys) and len(keys) > 100
    kk = dev(keys)
    assert torch.equal(a.export(kk), b.export(kk))
    a.close()
    b.close()
    comm.close()


# ==== SparseEmbedding ===============================================================================
@pytest.mark.parametrize("dtype,maximize", [("f32", False), ("f64", True)])
def test_sparse_embedding(lib, gpu, dtype, maximize):
    from swiftmpi_amd.nn import SparseEmbedding
    D = 6
    t = mk(lib, "w2v", D, dtype)
    emb = SparseEmbedding(t, maximize=maximize)
    assert not list(emb.parameters())
    ids = torch.tensor([[7, 9, 7, -1, 11], [9, 7, 13, 13, 7], [11, 15, 7, 9, 9]], dtype=torch.int64, device="cuda")
    rng = np.random.default_rng(8)
    w = tm.gen_grads(rng, 15, 2 * D, tm.DT[dtype]).reshape(3, 5, 2 * D)
    out = emb(ids)
    assert out.shape == (3, 5, 2 * D) and out.requires_grad
    flat = host(ids).reshape(-1).astype(np.uint64)  # -1 -> ~0
    m = tm.TableModel("w2v", D, dtype, tm.LR_RATE, seed=SEED)
    real = flat != PAD
    want = np.zeros((15, 2 * D), dtype=tm.DT[dtype])
    want[real] = m.pull(flat[real])
    assert tm.same_bits(host(out.detach()).reshape(15, -1), want)
    assert t.size() == 5
    loss = (out * dev(w)).sum()
    loss.backward()  # the table's push rule runs here
    sign = 1.0 if maximize else -1.0
    assert len(dm.push_dup(m, flat, w.reshape(15, -1), "sum", sign)) == 0
    keys = np.array([7, 9, 11, 13, 15], dtype=np.uint64)
    tm.assert_rows_equal(host(t.export(dev(keys))), m.export(keys), "w2v", "after backward")
    with torch.no_grad():
        out2 = emb(ids)
    want2 = np.zeros_like(want)
    want2[real] = m.export(flat[real])[:, :2 * D]
    assert tm.same_bits(host(out2).reshape(15, -1), want2)
    t.close()
