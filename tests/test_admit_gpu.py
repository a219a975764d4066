"""Admission by count on the HBM table (swiftmpi_amd/csrc/swps_admit.h / swps_admit.hip, DESIGN.md
section 16) against the NumPy model of tests/admit_model.py.  Every comparison is equality of bits
or integers; tests/test_admit_cpu.py shows on the CPU that the inputs used here have no false admit
in the 2^16-cell sketch, many in the 64-cell one, and tell the two-pass rule from a per-key one.

Shapes: 1, 255, 257 and 5000 distinct keys per call are one thread, one block less one, one block
plus one and twenty blocks of the one-thread-per-key kernels (and of the scan's tiles).

Row order: the table's insert kernel hands out row indices from an atomic counter, so the order of
the rows WITHIN one inserting call is not defined (every older test compares `keys()` as a set).
Across calls it is: the keys admitted by call c occupy the rows after those of call c - 1.  `keys()`
is compared segment by segment, each segment as a set, which is everything the table defines.
"""
import functools

import numpy as np
import pytest
import torch

import admit_model as am
import bag_model as bm
import dup_model as dm
import table_model as tm

pytestmark = pytest.mark.gpu

SEED = am.SEED
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
E_BADKEY, E_STATE, E_UNSUPPORTED = -2, -6, -7


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).to("cuda")


def host(t):
    return t.cpu().numpy()


def mk(lib, layout="lr", D=1, dtype="f32", rule="adagrad", capacity=1 << 14, init="hash", **kw):
    return lib.Table(layout, dim=D, capacity=capacity, dtype=dtype, learning_rate=tm.LR_RATE, init=init, seed=SEED,
                     push_rule=rule, **kw)


def model_of(layout="lr", D=1, dtype="f32", min_count=2, width=1 << 16, rule="adagrad"):
    return am.AdmitModel(tm.TableModel(layout, D, dtype, tm.LR_RATE, 1e-6, rule, seed=SEED), min_count, width, SEED)


def check_keys(t, segments):
    """t.keys(): the segments' keys in segment order, each segment in any order (module docstring)."""
    got = t.keys()
    assert len(got) == sum(len(s) for s in segments)
    o = 0
    for s in segments:
        assert np.array_equal(np.sort(got[o:o + len(s)]), np.sort(s))
        o += len(s)


def counters(t):
    a = t.admission()
    return {k: a[k] for k in ("tested", "admitted", "refused")}


def check_lookup(t, m, ids, segments):
    """One gated lookup on table and model: found, values, row order, cells, counters."""
    want_vals, want_found = m.lookup(ids)
    vals, found = t.lookup(dev(ids), return_found=True)
    assert np.array_equal(host(found), want_found)
    assert tm.same_bits(host(vals), want_vals)
    segments.append(m.last_admitted)
    check_keys(t, segments)
    assert np.array_equal(t.admission_cells(), m.cells)
    assert counters(t) == m.counters()


@functools.lru_cache(maxsize=None)
def the_case(nu, min_count):
    return am.stream_case(nu, min_count)


# ==== the stream ====================================================================================
@pytest.mark.parametrize("width", am.WIDTHS)
@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
@pytest.mark.parametrize("nu", am.NUS)
@pytest.mark.parametrize("layout,D,dtype", am.LAYOUTS)
def test_stream_equals_model(lib, gpu, layout, D, dtype, nu, min_count, width):
    """min_count + 1 calls in sequence with repeats and -1 padding; after every call found, values
    (refused = zero), row order, the cells and the three counters are the model's."""
    case = the_case(nu, min_count)
    t = mk(lib, layout, D, dtype, admit_min_count=min_count, admit_width=width)
    m = model_of(layout, D, dtype, min_count, width)
    assert t.admission() == dict(min_count=min_count, width=width, depth=4, tested=0, admitted=0, refused=0)
    segments = []
    for c, ids in enumerate(case["calls"]):
        # the padding id is refused by an inserting lookup as by swps_pull, after the call's work
        with pytest.raises(lib.SwpsError) as e:
            t.lookup(dev(ids))
        assert e.value.code == E_BADKEY and "empty key" in str(e.value)
        want_vals, want_found = m.lookup(ids)
        segments.append(m.last_admitted)
        check_keys(t, segments)
        assert np.array_equal(t.admission_cells(), m.cells), c
        assert counters(t) == m.counters(), c
        # the values and flags, without inserting: what the call above returned rows for
        vals, found = t.lookup(dev(ids), insert=False, return_found=True)
        assert np.array_equal(host(found), want_found), c
        assert tm.same_bits(host(vals), want_vals), c
    t.barrier()
    assert t.size() == m.table.size()
    t.close()


@pytest.mark.parametrize("width", am.WIDTHS)
@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
@pytest.mark.parametrize("nu", am.NUS)
def test_stream_without_padding_returns_the_model_s_values(lib, gpu, nu, min_count, width):
    """The same stream with the padding taken out: the inserting call itself returns found and the
    values (W2V f32, D = 8: 16-byte lanes)."""
    case = the_case(nu, min_count)
    t = mk(lib, "w2v", 8, "f32", admit_min_count=min_count, admit_width=width)
    m = model_of("w2v", 8, "f32", min_count, width)
    segments = []
    for ids in case["calls"]:
        check_lookup(t, m, ids[ids != PAD], segments)
    t.barrier()
    t.close()


@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
def test_admitted_in_the_call_or_on_call_number_min_count(lib, gpu, min_count):
    rng = np.random.default_rng(21)
    often, once = tm.gen_keys(rng, 2)
    t = mk(lib, admit_min_count=min_count, admit_width=1 << 16)
    for c in range(1, min_count + 2):
        ids = np.array([once] + ([often] * min_count if c == 1 else []), dtype=np.uint64)
        _, found = t.lookup(dev(ids), return_found=True)
        f = host(found).tolist()
        assert f[0] == (1 if c >= min_count else 0), c
        assert f[1:] == [1] * (len(ids) - 1)
    assert counters(t) == dict(tested=min_count + 1, admitted=2, refused=min_count - 1)
    t.close()


# ==== the sketch ====================================================================================
def test_saturation(lib, gpu):
    """Cells loaded at 2^32 - 3 stop at 2^32 - 1, whatever collides in them."""
    t = mk(lib, admit_min_count=5, admit_width=64)
    m = model_of(min_count=5, width=64)
    full = np.full((4, 64), 2 ** 32 - 3, dtype=np.uint32)
    t.admission_load(full)
    m.cells[:] = full
    assert np.array_equal(t.admission_cells(), full)
    keys = tm.gen_keys(np.random.default_rng(22), 200)
    ids = np.random.default_rng(23).permutation(np.repeat(keys, 5))
    check_lookup(t, m, ids, [])
    cells = t.admission_cells()
    assert cells.max() == 2 ** 32 - 1 and set(np.unique(cells).tolist()) <= {2 ** 32 - 3, 2 ** 32 - 1}
    t.close()


def test_decay_and_checkpoint(lib, gpu):
    t = mk(lib, admit_min_count=5, admit_width=64)
    m = model_of(min_count=5, width=64)
    keys = tm.gen_keys(np.random.default_rng(24), 300)
    segments = []
    check_lookup(t, m, np.repeat(keys[:100], 3), segments)
    saved = t.admission_cells()
    assert saved.dtype == np.uint32 and saved.shape == (4, 64) and saved.any()
    t.admission_decay(1)
    m.decay(1)
    assert np.array_equal(t.admission_cells(), saved >> np.uint32(1)) and np.array_equal(m.cells, saved >> np.uint32(1))
    check_lookup(t, m, np.repeat(keys[100:200], 2), segments)  # the halved counts gate the next call
    t.admission_decay(32)
    m.decay(32)
    assert not t.admission_cells().any()
    assert counters(t) == m.counters()  # decay keeps the counters
    t.admission_load(saved)
    m.cells = saved.copy()
    check_lookup(t, m, keys[200:], segments)
    with pytest.raises(lib.SwpsError) as e:
        t.admission_load(np.zeros((4, 128), dtype=np.uint32))
    assert e.value.code == -5
    # setting it again zeroes the cells and the counters; off frees the sketch
    t.set_admission(5, 128)
    assert t.admission() == dict(min_count=5, width=128, depth=4, tested=0, admitted=0, refused=0)
    assert t.admission_cells().shape == (4, 128) and not t.admission_cells().any()
    t.set_admission(1)
    assert t.admission()["min_count"] == 0
    for call in (t.admission_cells, lambda: t.admission_decay(1), lambda: t.admission_load(saved)):
        with pytest.raises(lib.SwpsError) as e:
            call()
        assert e.value.code == E_STATE
    t.close()


def test_sketch_survives_erase_growth_and_save(lib, gpu, tmp_path):
    """The sketch is no part of the rows: reserve / shrink / erase / prune / save / restore leave it
    alone; an erased key keeps its counts and is re-admitted at once."""
    t = mk(lib, "w2v", 8, "f32", capacity=512, admit_min_count=2, admit_width=64)
    keys = tm.gen_keys(np.random.default_rng(25), 300)
    t.lookup(dev(np.repeat(keys[:200], 2)))
    t.lookup(dev(keys[200:]))
    cells, stats = t.admission_cells(), t.admission()
    assert t.size() >= 200
    t.reserve(2048)
    assert t.erase(dev(keys[:50])) == 50
    t.push_dup(dev(keys[50:200]), torch.ones(150, 16, device="cuda"))
    t.prune(0.0)  # the keys that never received a gradient
    assert t.size() == 150
    t.shrink(1024)
    path = str(tmp_path / "t.swps")
    t.save(path)
    t.restore(path)
    assert np.array_equal(t.admission_cells(), cells) and t.admission() == stats
    _, found = t.lookup(dev(keys[:50]), return_found=True)  # one occurrence each: the old counts admit them
    assert host(found).all()
    t.close()


# ==== bags ==========================================================================================
@pytest.mark.parametrize("mode,weighted", [("sum", False), ("mean", False), ("sum", True)])
@pytest.mark.parametrize("layout,D,dtype", am.LAYOUTS)
def test_lookup_bag_gated(lib, gpu, layout, D, dtype, mode, weighted):
    """Refused members contribute zero and still count in the mean; the result is bit-identical to
    lookup_bag(insert=False) after lookup(insert=True) of the same ids on a twin table."""
    rng = np.random.default_rng([26, D])
    pool = tm.gen_keys(rng, 400)
    a = mk(lib, layout, D, dtype, admit_min_count=2, admit_width=1 << 16)
    b = mk(lib, layout, D, dtype, admit_min_count=2, admit_width=1 << 16)
    m = model_of(layout, D, dtype, 2, 1 << 16)
    for call in range(3):
        ids = pool[rng.integers(0, 400, 700)]
        ids[::37] = PAD
        off = np.array([0, 0, 1, 5, 300, 300, 700], dtype=np.int64)
        w = rng.uniform(-2.0, 2.0, len(ids)) if weighted else None
        vals, found = m.lookup(ids)
        assert 0 < found[ids != PAD].sum() < (ids != PAD).sum()  # refused members are really in the bags
        want = bm.pool(vals, ids != PAD, off, w, mode)
        got = a.lookup_bag(dev(ids), dev(off), None if w is None else dev(w), mode)
        assert tm.same_bits(host(got), want), call
        b.lookup(dev(ids[ids != PAD]))
        twin = b.lookup_bag(dev(ids), dev(off), None if w is None else dev(w), mode, insert=False)
        assert torch.equal(got, twin)
        assert np.array_equal(a.admission_cells(), m.cells) and np.array_equal(b.admission_cells(), m.cells)
        assert counters(a) == counters(b) == m.counters()
        assert a.size() == b.size() == m.table.size()
    a.barrier()
    a.close()
    b.close()


# ==== pushes ========================================================================================
@pytest.mark.parametrize("layout,D,dtype", am.LAYOUTS)
def test_pushes_skip_refused_ids(lib, gpu, layout, D, dtype):
    """push_dup / push_bag with refused ids leave barrier() clean and the admitted rows equal to the
    model's; the same calls on a table with admission off still latch SWPS_E_BADKEY."""
    rng = np.random.default_rng([27, D])
    pool = tm.gen_keys(rng, 300)
    G = tm.DT["f64" if layout == "w2v" else "f32"]
    t = mk(lib, layout, D, dtype, admit_min_count=2, admit_width=1 << 16)
    off_table = mk(lib, layout, D, dtype)
    m = model_of(layout, D, dtype, 2, 1 << 16)
    ids = np.concatenate([np.repeat(pool[:100], 2), pool[100:]])
    ids = rng.permutation(np.concatenate([ids, np.full(9, PAD, dtype=np.uint64)]))
    real = ids[ids != PAD]
    t.lookup(dev(real))
    m.lookup(real)
    off_table.lookup(dev(pool[:100]))
    assert t.size() == 100
    g = tm.gen_grads(rng, len(ids), t.push_elems, G)
    t.push_dup(dev(ids), dev(g), "mean", -1.0)
    assert sorted(dm.push_dup(m.table, ids, g, "mean", -1.0).tolist()) == sorted(pool[100:].tolist())
    off = np.array([0, 3, 3, 200, len(ids)], dtype=np.int64)
    bg = tm.gen_grads(rng, 4, t.push_elems, G)
    t.push_bag(dev(ids), dev(off), dev(bg), mode="mean")
    assert len(bm.push_bag(m.table, ids, off, bg, None, "mean")) == 200
    t.barrier()  # nothing was latched
    tm.assert_rows_equal(host(t.export(dev(pool[:100]))), m.table.export(pool[:100]), layout, "gated pushes")
    assert t.size() == 100
    for call in (lambda: off_table.push_dup(dev(ids), dev(g), "mean", -1.0),
                 lambda: off_table.push_bag(dev(ids), dev(off), dev(bg), mode="mean")):
        with pytest.raises(lib.SwpsError) as e:
            call()
        assert e.value.code == E_BADKEY
    t.close()
    off_table.close()


# ==== growth and init order =========================================================================
def test_growth_counts_the_admitted_keys(lib, gpu):
    """Under a ceiling a call whose refused ids would have forced a growth moves nothing; the
    growths follow swps_grow_plan fed the ADMITTED count (every call ends synchronised, so the
    host's bound on the rows is the row count)."""
    rng = np.random.default_rng(28)
    pool = tm.gen_keys(rng, 600)
    t = mk(lib, "w2v", 8, "f32", capacity=4, max_capacity=1 << 12, admit_min_count=2, admit_width=1 << 16)
    m = model_of("w2v", 8, "f32", 2, 1 << 16)
    cap, growths = 4, 0
    calls = [pool[:300], pool[:3], pool[300:], np.concatenate([pool[:40], pool[300:310]]), pool]
    for c, ids in enumerate(calls):
        rows = m.table.size()
        m.lookup(ids)
        na = len(m.last_admitted)
        if na and na > cap - rows:
            nc, _ = lib.grow_plan(cap, 1 << 12, rows, na)
            if nc > cap:
                cap, growths = nc, growths + 1
        t.lookup(dev(ids))
        got = t.capacity()
        assert (got["capacity"], got["growths"]) == (cap, growths), (c, got)
        assert t.size() == m.table.size() and counters(t) == m.counters()
    assert growths >= 2
    u = mk(lib, "w2v", 8, "f32", capacity=4, max_capacity=1 << 12)
    u.lookup(dev(calls[0]))
    assert u.capacity()["growths"] == 1 and growths > 0  # the ungated table moved for the first call already
    t.close()
    u.close()


def test_flcg_draws_in_admitted_first_occurrence_order(lib, gpu):
    rng = np.random.default_rng(29)
    pool = tm.gen_keys(rng, 500)
    a = mk(lib, "lr", 1, "f32", init="flcg", admit_min_count=2, admit_width=1 << 16)
    b = mk(lib, "lr", 1, "f32", init="flcg")
    m = model_of(min_count=2, width=1 << 16)
    for call in range(4):
        ids = pool[rng.integers(0, 500, 600)]
        m.lookup(ids)
        a.lookup(dev(ids))
        if len(m.last_admitted):
            b.pull(dev(m.last_admitted))  # the ungated table draws in the order of its key list
    ks = m.keys()
    assert len(ks) > 300 and a.size() == b.size() == len(ks)
    ra, rb = host(a.export(dev(ks))), host(b.export(dev(ks)))
    assert tm.same_bits(ra, rb) and len(np.unique(ra[:, 0])) > 250  # draws, not one value
    a.close()
    b.close()


# ==== what is not gated =============================================================================
def test_pull_assign_restore_insert_regardless(lib, gpu, tmp_path):
    rng = np.random.default_rng(30)
    k = tm.gen_keys(rng, 90)
    t = mk(lib, "w2v", 3, "f64", admit_min_count=5, admit_width=64)
    t.pull(dev(k[:30]))
    assert t.size() == 30
    t.assign(dev(k[30:60]), dev(tm.gen_rows(rng, 30, "w2v", 3, np.float64)))
    assert t.size() == 60
    src = mk(lib, "w2v", 3, "f64")
    src.pull(dev(k[60:]))
    path = str(tmp_path / "s.swps")
    src.save(path)
    t.restore(path)
    assert t.size() == 90 and set(t.keys().tolist()) == set(k.tolist())
    t.pull_h(np.array([7, 8, 9], dtype=np.uint64))
    assert t.size() == 93
    assert counters(t) == dict(tested=0, admitted=0, refused=0) and not t.admission_cells().any()
    t.barrier()
    t.close()
    src.close()


def test_admission_off_is_the_table_it_was(lib, gpu):
    """A table whose admission was turned on and off again, given the same calls, is bit-identical
    to one on which set_admission was never called."""
    rng = np.random.default_rng(31)
    pool = tm.gen_keys(rng, 400)
    a = mk(lib, "w2v", 8, "f32", capacity=8, max_capacity=1 << 12)
    b = mk(lib, "w2v", 8, "f32", capacity=8, max_capacity=1 << 12, admit_min_count=5, admit_width=64)
    b.set_admission(0)
    c = mk(lib, "w2v", 8, "f32", capacity=8, max_capacity=1 << 12, admit_min_count=1)
    assert b.admission() == c.admission() == a.admission() == dict(min_count=0, width=0, depth=4, tested=0,
                                                                   admitted=0, refused=0)
    for r in range(3):
        ids = pool[rng.integers(0, 100 * (r + 1), 500)]
        off = np.array([0, 100, 100, 500], dtype=np.int64)
        g = tm.gen_grads(rng, len(ids), 16, np.float32)
        outs = []
        for t in (a, b, c):
            v, f = t.lookup(dev(ids[:250]), return_found=True)
            bag = t.lookup_bag(dev(ids), dev(off), mode="mean")
            t.push_dup(dev(ids), dev(g), "sum", -1.0)
            outs.append((v, f, bag))
        for o in outs[1:]:
            assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
    unknown = dev(np.array([12345], dtype=np.uint64))
    for t in (a, b, c):
        with pytest.raises(lib.SwpsError) as e:
            t.push_dup(unknown, torch.ones(1, 16, device="cuda"))
        assert e.value.code == E_BADKEY
    ks = np.sort(a.keys())
    for t in (b, c):
        assert np.array_equal(np.sort(t.keys()), ks) and t.capacity() == a.capacity()
        assert torch.equal(t.export(dev(ks)), a.export(dev(ks)))
        assert t.admission()["tested"] == 0
    for t in (a, b, c):
        t.close()


def test_routed_tables_are_refused_both_ways(lib, gpu, gloo1):
    from swiftmpi_amd.comm import Comm
    comm = Comm.host()
    a = mk(lib)
    a.route(comm, frag_num=1000)
    with pytest.raises(lib.SwpsError) as e:
        a.set_admission(2, 64)
    assert e.value.code == E_UNSUPPORTED and "swps_table_route" in str(e.value)
    assert a.admission()["min_count"] == 0
    a.set_admission(0)  # turning it off is no change: accepted
    b = mk(lib, admit_min_count=2, admit_width=64)
    with pytest.raises(lib.SwpsError) as e:
        b.route(comm, frag_num=1000)
    assert e.value.code == E_UNSUPPORTED and "swps_table_set_admission" in str(e.value)
    assert b.admission()["min_count"] == 2
    a.finish()
    a.close()
    b.close()
    comm.close()


# ==== the torch modules =============================================================================
def module_ids(rng):
    """[B, L] ids: keys 0..19 occur twice or more (admitted at min_count 2), 20..59 once (refused)."""
    pool = tm.gen_keys(rng, 60).view(np.int64)
    pool = pool[pool != -1]
    flat = np.concatenate([np.repeat(pool[:20], rng.integers(2, 5, 20)), pool[20:]])
    flat = rng.permutation(flat)
    L = 5
    flat = flat[:len(flat) // L * L]
    often = np.array([k for k in pool[:20] if (flat == k).sum() >= 2])
    rare = np.array([k for k in pool if 0 < (flat == k).sum() < 2])
    assert len(often) > 10 and len(rare) > 10
    return flat.reshape(-1, L), often.view(np.uint64), rare.view(np.uint64)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_sparse_embedding_over_a_gated_table(lib, gpu, dtype):
    from swiftmpi_amd.nn import SparseEmbedding
    D = 4
    rng = np.random.default_rng(32)
    ids_h, often, rare = module_ids(rng)
    ids = torch.as_tensor(ids_h).to("cuda")
    a = mk(lib, "w2v", D, dtype, admit_min_count=2, admit_width=1 << 16)
    b = mk(lib, "w2v", D, dtype)
    b.lookup(dev(often))  # pre-filled with exactly the admitted keys (hash init: the same rows)
    C = dev(tm.gen_grads(rng, ids_h.size, 2 * D, tm.DT[dtype]).reshape(*ids_h.shape, 2 * D))
    out = SparseEmbedding(a)(ids)
    refused = torch.as_tensor(np.isin(ids_h.view(np.uint64), rare)).to("cuda")
    assert a.size() == len(often) and bool(refused.any())
    assert not out[refused].any() and bool(out[~refused].abs().sum(-1).gt(0).all())
    (out * C).sum().backward()
    a.barrier()  # the refused ids' gradients were skipped, nothing latched
    assert a.size() == len(often)
    (SparseEmbedding(b)(ids) * C).sum().backward()
    assert torch.equal(a.export(dev(often)), b.export(dev(often)))
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_sparse_embedding_bag_over_a_gated_table(lib, gpu, mode):
    from swiftmpi_amd.nn import SparseEmbeddingBag
    D = 4
    rng = np.random.default_rng(33)
    ids_h, often, rare = module_ids(rng)
    ids = torch.as_tensor(ids_h).to("cuda")
    B, L = ids_h.shape
    a = mk(lib, "w2v", D, "f32", admit_min_count=2, admit_width=1 << 16)
    b = mk(lib, "w2v", D, "f32")
    b.lookup(dev(often))
    m = model_of("w2v", D, "f32", 2, 1 << 16)
    flat = ids_h.reshape(-1).view(np.uint64)
    vals, found = m.lookup(flat)
    C = dev(tm.gen_grads(rng, B, 2 * D, np.float32))
    out = SparseEmbeddingBag(a, mode=mode)(ids)
    want = bm.pool(vals, np.ones(len(flat), dtype=bool), np.arange(B + 1) * L, None, mode)
    assert tm.same_bits(host(out.detach()), want)  # refused members: zero rows that count in the mean
    assert a.size() == len(often) == m.table.size()
    (out * C).sum().backward()
    a.barrier()
    (SparseEmbeddingBag(b, mode=mode)(ids) * C).sum().backward()
    assert torch.equal(a.export(dev(often)), b.export(dev(often)))
    a.close()
    b.close()
