"""The pooled calls of the HBM table (swiftmpi_amd/csrc/swps_bag.hip: swps_lookup_bag, swps_push_bag,
their host forms and swiftmpi_amd.nn.SparseEmbeddingBag) against the NumPy model of
tests/bag_model.py.  Every comparison is bit equality; tests/test_bag_cpu.py shows on the CPU that
the model and the inputs used here tell a wrong order or operand from the right one.

Dispatch, as read from the source:
  forward   one thread per bag / item (LR, and W2V values under 16 bytes), 16-B lanes (row and pull
            bytes multiples of 16: f32 even D, every f64 W2V table), scalar lanes (f32 odd D); D = 100
            is one trip of the 64 lanes at f32, D = 300 has a tail trip; bags of <= 128 positions in
            one wave, longer bags as (bag, chunk) items; the member loop runs four rows at a time
            with a scalar tail (bag lengths 1, 2, 3 and 127 take the tail)
  backward  the (run, chunk) reduce of the repeated-key push with the bag's gradient row as source:
            E = 16 / sizeof(G) elements per lane when 2 D % E == 0, else 1
"""
import functools

import numpy as np
import pytest
import torch

import bag_model as bm
import dup_model as dm
import table_model as tm

pytestmark = pytest.mark.gpu

SEED = 11
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
E_BADKEY, E_CFG = -2, -5


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).to("cuda")


def host(t):
    return t.cpu().numpy()


def mk(lib, layout, D, dtype, rule="adagrad", capacity=4096, init="hash", **kw):
    return lib.Table(layout, dim=D, capacity=capacity, dtype=dtype, learning_rate=tm.LR_RATE, init=init, seed=SEED,
                     push_rule=rule, **kw)


@functools.lru_cache(maxsize=None)
def the_case(layout, D, dtype):
    return bm.bag_case(layout, D, dtype)


@functools.lru_cache(maxsize=None)
def want_forward(layout, D, dtype, mode, weighted):
    out = bm.forward(the_case(layout, D, dtype), mode, weighted)
    out.setflags(write=False)
    return out


def table_of(lib, case, rule="adagrad"):
    t = mk(lib, case["layout"], case["D"], case["dtype"], rule)
    t.assign(dev(case["keys"]), dev(case["rows"]))
    return t


TABLES = [("w2v", D, dt) for D in (4, 5, 6, 100, 300) for dt in ("f32", "f64")] + [("lr", 1, "f32"), ("lr", 1, "f64")]
VARIANTS = [("sum", False), ("mean", False), ("sum", True)]


# ==== forward =======================================================================================
@pytest.mark.parametrize("layout,D,dtype", TABLES)
def test_lookup_bag_equals_model(lib, gpu, layout, D, dtype):
    """Bag lengths 0, 1, 2, 3, 127, 128, 129, 257, 385 and 3000; empty bags at the start, the end and
    adjacent; padding at the head, middle and tail, a whole chunk of it, a bag of nothing else; keys
    repeated inside and across bags; column 0 carries the MAG / CHUNKY / MEAN3 / NEGZ / W32 devices."""
    case = the_case(layout, D, dtype)
    t = table_of(lib, case)
    ids, off = dev(case["ids"]), dev(case["offsets"])
    wire = np.float64 if layout == "w2v" else np.float32
    for mode, weighted in VARIANTS:
        want = want_forward(layout, D, dtype, mode, weighted)
        w = case["weights"] if weighted else None
        got = t.lookup_bag(ids, off, None if w is None else dev(w), mode)
        assert got.shape == (len(case["offsets"]) - 1, t.pull_elems)
        assert tm.same_bits(host(got), want), (mode, weighted, np.argwhere(tm.bits(host(got)) != tm.bits(want))[:4])
        # fp32 weights are converted on the device: the same call as with their fp64 values
        if weighted and D == 6:
            w32 = w.astype(np.float32)
            a = t.lookup_bag(ids, off, dev(w32), mode)
            assert torch.equal(a, t.lookup_bag(ids, off, dev(w32.astype(np.float64)), mode))
        # the host form returns the wire type
        if D in (5, 6, 1):
            gh = t.lookup_bag(case["ids"], case["offsets"], w, mode)
            assert tm.same_bits(gh, want.astype(wire))
    assert t.size() == len(case["keys"])
    t.close()


def test_lookup_bag_inserts_grows_and_counts_distinct_keys(lib, gpu):
    """insert=True on an empty table: the model over hash_init, size() = the distinct count; a
    small table under a ceiling grows as `lookup` of the same ids would."""
    case = the_case("w2v", 6, "f32")
    ids, off = case["ids"], case["offsets"]
    distinct = len(np.unique(ids[ids != PAD]))
    m = tm.TableModel("w2v", 6, "f32", tm.LR_RATE, seed=SEED)
    want = bm.lookup_bag(m, ids, off, None, "mean", True)
    assert m.size() == distinct
    t = mk(lib, "w2v", 6, "f32")
    assert tm.same_bits(host(t.lookup_bag(dev(ids), dev(off), mode="mean")), want)
    assert t.size() == distinct
    t.close()
    a = mk(lib, "w2v", 6, "f32", capacity=4, max_capacity=1 << 16)
    b = mk(lib, "w2v", 6, "f32", capacity=4, max_capacity=1 << 16)
    got = a.lookup_bag(dev(ids), dev(off), mode="mean")
    b.lookup(dev(ids[ids != PAD]))
    assert tm.same_bits(host(got), want)
    assert a.size() == b.size() == distinct
    assert a.capacity() == b.capacity() and a.capacity()["capacity"] <= max(8, distinct)  # not n = 4600
    a.close()
    b.close()


def test_lookup_bag_flcg_draws_in_first_occurrence_order(lib, gpu):
    rng = np.random.default_rng(3)
    pool = tm.gen_keys(rng, 200)
    ids = pool[rng.integers(0, 200, 1500)]
    ids[::41] = PAD
    off = np.array([0, 0, 700, 701, 1500], dtype=np.int64)
    uniq, inv, _ = dm.coalesce(ids)
    a = mk(lib, "lr", 1, "f32", init="flcg")
    b = mk(lib, "lr", 1, "f32", init="flcg")
    got = host(a.lookup_bag(dev(ids), dev(off)))
    rows = host(b.pull(dev(uniq)))
    assert len(np.unique(rows)) > 150  # draws, not one value
    vals = np.zeros((len(ids), 1), dtype=np.float32)
    vals[ids != PAD] = rows[inv[ids != PAD]]
    assert tm.same_bits(got, bm.pool(vals, ids != PAD, off))
    a.close()
    b.close()


def test_lookup_bag_without_insert_counts_absent_keys(lib, gpu):
    rng = np.random.default_rng(5)
    t = mk(lib, "w2v", 6, "f64")
    keys = tm.gen_keys(rng, 30)
    rows = tm.gen_rows(rng, 30, "w2v", 6, np.float64)
    t.assign(dev(keys[:20]), dev(rows[:20]))
    ids = keys[rng.integers(0, 30, 400)]
    ids[::19] = PAD
    ids[:3] = [keys[25], keys[0], keys[26]]  # an absent key leads a bag: the chain starts from its +0.0
    off = np.array([0, 3, 3, 150, 400], dtype=np.int64)
    m = tm.TableModel("w2v", 6, "f64", tm.LR_RATE)
    m.assign(keys[:20], rows[:20])
    for mode in ("sum", "mean"):
        want = bm.lookup_bag(m, ids, off, None, mode, insert=False)
        assert tm.same_bits(host(t.lookup_bag(dev(ids), dev(off), mode=mode, insert=False)), want)
    # the absent keys count in the mean: bag 0 divides by 3
    assert tm.same_bits(want[0], (rows[0, :12] / np.float64(3)))
    assert t.size() == 20 and m.size() == 20
    t.barrier()  # nothing was latched
    t.close()


# ==== backward ======================================================================================
PUSH_CASES = [(l, D, dt, gt) + v for (l, D, dt) in TABLES for gt in (("f32", "f64") if l == "w2v" else ("f32",))
              for v in (("sum", False, "adagrad", 1.0), ("mean", False, "sgd", -1.0), ("sum", True, "adagrad", -1.0))]


@pytest.mark.parametrize("layout,D,dtype,gtype,mode,weighted,rule,scale", PUSH_CASES)
def test_push_bag_equals_model(lib, gpu, layout, D, dtype, gtype, mode, weighted, rule, scale):
    """Two chained calls (the accumulators matter) on the forward's ids and bags."""
    case = the_case(layout, D, dtype)
    t = table_of(lib, case, rule)
    ids, off = dev(case["ids"]), dev(case["offsets"])
    w = dev(case["weights"]) if weighted else None
    for G in bm.bag_grads(case, gtype):
        t.push_bag(ids, off, dev(G), w, mode, scale)
    want = bm.backward(case, gtype, rule, mode, weighted, scale)
    tm.assert_rows_equal(host(t.export(dev(case["keys"]))), want, layout, "push_bag")
    t.close()


@pytest.mark.parametrize("D,dtype,gtype,mode,weighted", [(6, "f32", "f32", "mean", False), (5, "f64", "f64", "sum", True),
                                                         (300, "f32", "f64", "mean", False)])
def test_push_bag_is_push_dup_of_the_expanded_matrix(lib, gpu, D, dtype, gtype, mode, weighted):
    """On a W2V table swps_push_bag leaves the table bit-identical to swps_push_dup fed the
    expanded fp64 [n][push] matrix; the host form does the same."""
    case = the_case("w2v", D, dtype)
    a, b, c = (table_of(lib, case) for _ in range(3))
    ids, off = dev(case["ids"]), dev(case["offsets"])
    w = case["weights"] if weighted else None
    G = bm.bag_grads(case, gtype)[0]
    a.push_bag(ids, off, dev(G), None if w is None else dev(w), mode, -1.0)
    b.push_dup(ids, dev(bm.expand(G, case["ids"], case["offsets"], w, mode)), "sum", -1.0)
    c.push_bag(case["ids"], case["offsets"], G, w, mode, -1.0)  # host arrays, wire type
    dk = dev(case["keys"])
    assert torch.equal(a.export(dk), b.export(dk))
    assert torch.equal(c.export(dk), b.export(dk))
    for t in (a, b, c):
        t.close()


def test_push_bag_unknown_key_is_reported_after_the_others(lib, gpu):
    case = the_case("w2v", 6, "f32")
    t = table_of(lib, case)
    ids = case["ids"].copy()
    ids[[1, 2000]] = np.uint64(424242)
    G = bm.bag_grads(case, "f64")[0]
    with pytest.raises(lib.SwpsError) as e:
        t.push_bag(dev(ids), dev(case["offsets"]), dev(G), mode="mean")
    assert e.value.code == E_BADKEY
    m = bm.case_model(case)
    assert bm.push_bag(m, ids, case["offsets"], G, None, "mean").tolist() == [424242]
    tm.assert_rows_equal(host(t.export(dev(case["keys"]))), m.export(case["keys"]), "w2v", "after the unknown key")
    assert t.size() == len(case["keys"])
    t.close()


def test_inputs_still_being_written_by_torch_are_waited_for(lib, gpu):
    """The bag gradient (and the weights) are the output of torch kernels queued just before the
    call, on torch's default stream, as in a backward pass: the call is ordered after them."""
    rng = np.random.default_rng(12)
    V, D, B, L = 2000, 100, 2048, 16
    keys = tm.gen_keys(rng, V)
    ids = dev(keys[rng.integers(0, V, B * L)])
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * L
    a, b = mk(lib, "w2v", D, "f32"), mk(lib, "w2v", D, "f32")
    for t in (a, b):
        t.lookup(dev(keys))
    x = torch.randn(8192, 2048, device="cuda")

    def grads():  # some milliseconds of element-wise kernels (deterministic), then the slice
        z = x
        for _ in range(40):
            z = torch.sin(z) * 1.0001
        return (z[:B, :2 * D] * 0.1).contiguous()
    want_G = grads()
    torch.cuda.synchronize()
    b.push_bag(ids, off, want_G)  # complete inputs
    G = grads()  # queued, not waited for
    a.push_bag(ids, off, G)
    assert torch.equal(G, want_G)
    dk = dev(keys)
    assert torch.equal(a.export(dk), b.export(dk))
    a.close()
    b.close()


# ==== refusals ======================================================================================
@pytest.mark.parametrize("what", ["first", "decrease", "last"])
def test_bad_offsets_leave_the_table_untouched(lib, gpu, what):
    rng = np.random.default_rng(9)
    t = mk(lib, "w2v", 6, "f32")
    keys = tm.gen_keys(rng, 40)
    t.lookup(dev(keys[:20]))
    before = t.export(dev(keys[:20])).clone()
    ids = keys[rng.integers(0, 40, 300)]  # half of them absent: an insert would show in size()
    off = np.array([0, 10, 10, 140, 200, 300], dtype=np.int64)
    bad = {"first": (0, 1, 0), "decrease": (3, 5, 2), "last": (5, 299, 4)}[what]
    off[bad[0]] = bad[1]
    G = torch.ones(5, 12, device="cuda")
    for call in (lambda: t.lookup_bag(dev(ids), dev(off)), lambda: t.push_bag(dev(ids), dev(off), G),
                 lambda: t.lookup_bag(ids, off), lambda: t.push_bag(ids, off, host(G))):
        with pytest.raises(lib.SwpsError) as e:
            call()
        assert e.value.code == E_CFG and ("bad bag %d" % bad[2]) in str(e.value), str(e.value)
    assert t.size() == 20
    assert torch.equal(t.export(dev(keys[:20])), before)
    t.barrier()  # nothing was latched
    # python-side refusals and the empty calls
    with pytest.raises(ValueError):
        t.lookup_bag(dev(ids), dev(off), mode="max")
    with pytest.raises(lib.SwpsError) as e:
        t.lookup_bag(dev(ids), dev(np.array([0, 300])), torch.ones(300, device="cuda"), mode="mean")
    assert e.value.code == E_CFG
    none = dev(ids[:0])
    assert t.lookup_bag(none, dev(np.array([0]))).shape == (0, 12)
    z = t.lookup_bag(none, dev(np.array([0, 0, 0])), mode="mean")
    assert tm.same_bits(host(z), np.zeros((2, 12), dtype=np.float32))
    t.push_bag(none, dev(np.array([0, 0, 0])), G[:2])
    assert t.size() == 20
    t.close()


# ==== SparseEmbeddingBag ============================================================================
@pytest.mark.parametrize("dtype,maximize", [("f32", False), ("f64", True)])
def test_sparse_embedding_bag_equals_sparse_embedding_summed(lib, gpu, dtype, maximize):
    """sum, no weights, 2-D ids without padding, loss (out * C).sum(): the same rows, bit for bit, as
    SparseEmbedding(ids).sum(1) on a twin table IF the two sums agree; the forward is compared with
    the model (torch's sum has no defined order), the backward with the twin."""
    from swiftmpi_amd.nn import SparseEmbedding, SparseEmbeddingBag
    D, B, L = 6, 7, 5
    rng = np.random.default_rng(8)
    ids = torch.as_tensor(rng.integers(1, 12, (B, L))).to("cuda")
    C = dev(tm.gen_grads(rng, B, 2 * D, tm.DT[dtype]))
    a, b = mk(lib, "w2v", D, dtype), mk(lib, "w2v", D, dtype)
    bag, emb = SparseEmbeddingBag(a, maximize=maximize), SparseEmbedding(b, maximize=maximize)
    assert not list(bag.parameters())
    out = bag(ids)
    assert out.shape == (B, 2 * D) and out.requires_grad
    m = tm.TableModel("w2v", D, dtype, tm.LR_RATE, seed=SEED)
    flat = host(ids).reshape(-1).astype(np.uint64)
    off = np.arange(B + 1) * L
    assert tm.same_bits(host(out.detach()), bm.lookup_bag(m, flat, off))
    (out * C).sum().backward()  # the table's push rule runs here
    (emb(ids).sum(1) * C).sum().backward()
    keys = dev(np.unique(flat))
    assert a.size() == b.size() == keys.numel()
    assert torch.equal(a.export(keys), b.export(keys))
    sign = 1.0 if maximize else -1.0
    assert len(bm.push_bag(m, flat, off, host(C), None, "sum", sign)) == 0
    tm.assert_rows_equal(host(a.export(keys)), m.export(host(keys).view(np.uint64)), "w2v", "after backward")
    a.close()
    b.close()


def test_sparse_embedding_bag_forms(lib, gpu):
    """1-D ids with torch's start offsets / include_last_offset, the mean, padding in 2-D ids and
    per-sample weights, against the model."""
    from swiftmpi_amd.nn import SparseEmbeddingBag
    D = 4
    t = mk(lib, "w2v", D, "f32")
    m = tm.TableModel("w2v", D, "f32", tm.LR_RATE, seed=SEED)
    ids = torch.tensor([3, 5, 3, 8, 9, 5, 5], dtype=torch.int64, device="cuda")
    flat = host(ids).astype(np.uint64)
    starts = torch.tensor([0, 2, 2, 6], dtype=torch.int64, device="cuda")
    want = bm.lookup_bag(m, flat, [0, 2, 2, 6, 7], None, "mean")
    mean = SparseEmbeddingBag(t, mode="mean")
    assert tm.same_bits(host(mean(ids, starts).detach()), want)
    last = SparseEmbeddingBag(t, mode="mean", include_last_offset=True)
    assert tm.same_bits(host(last(ids, torch.cat([starts, starts.new_tensor([7])])).detach()), want)
    ids2 = torch.tensor([[3, -1, 5], [-1, -1, -1], [9, 9, -1]], dtype=torch.int64, device="cuda")
    f2 = host(ids2).reshape(-1).astype(np.uint64)
    assert tm.same_bits(host(mean(ids2).detach()), bm.lookup_bag(m, f2, [0, 3, 6, 9], None, "mean"))
    w = torch.tensor([[0.5, 7.0, -2.0], [1.0, 1.0, 1.0], [0.1, 0.2, 0.3]], device="cuda")
    summ = SparseEmbeddingBag(t)
    out = summ(ids2, per_sample_weights=w)
    w64 = host(w).astype(np.float64).reshape(-1)
    assert tm.same_bits(host(out.detach()), bm.lookup_bag(m, f2, [0, 3, 6, 9], w64))
    C = torch.ones_like(out)
    (out * C).sum().backward()
    assert len(bm.push_bag(m, f2, [0, 3, 6, 9], host(C), w64, "sum", -1.0)) == 0
    keys = np.array([3, 5, 8, 9], dtype=np.uint64)
    tm.assert_rows_equal(host(t.export(dev(keys))), m.export(keys), "w2v", "weighted backward")
    with pytest.raises(ValueError):
        summ(ids2, per_sample_weights=w.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        mean(ids2, per_sample_weights=w)
    t.close()
