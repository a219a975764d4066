"""The parameter shard's kernels (swiftmpi_amd/csrc/swps_table.hip) bit for bit against the
NumPy model of tests/table_model.py, at every kernel form the dispatch code selects.

Every comparison is bit equality (table_model.assert_rows_equal / same_bits): the library is
built with -ffp-contract=off and each push step is a chain of single IEEE operations that
NumPy repeats on the CPU.  tests/test_table_model_cpu.py shows on the CPU that the model and
the inputs below tell a wrong source order, a missing rounding, a re-association and a
one-ulp error from the right result.

Dispatch, as read from the source (E = elements per 16-byte lane access, 64 lanes per row):
  k_push_w2v<T, G, E>        E = 16 / sizeof(T) when D % E == 0, else 1; a second loop trip
                             when D / E > 64 (f32: D > 256 at E = 4, f64: D > 128 at E = 2,
                             D > 64 at E = 1)
  table_copy_pull            k_copy_rows_out_t   pull_elems <= 4 and under 16 bytes: f32 D = 1, LR
                             k_copy_rows_out16   row and pull bytes multiples of 16: f32 even D,
                                                 every f64 W2V table
                             k_copy_rows_out     the rest: f32 odd D >= 3
  table_push_sources         one source: k_push_w2v / k_push_lr, or k_push_w2v_multi_t<NCH>
                             with pos_s == nullptr; several: k_push_keys, the radix sort, then
                             k_push_w2v_multi_t<NCH> (f32 rows, f32 payload, D = 256 NCH + tail,
                             1 <= NCH <= 3, 1 <= tail <= 64), k_push_w2v_multi<T, G, E> or
                             k_push_lr_multi<T>

What one process cannot reach (asserted below where it can be): the W2V app context refuses
D % E != 0 and D > 1024 (f32) / 512 (f64), so the served path never sees D = 1, 3, 5, 65,
257, 321 or 1028 (the slice kernel's misaligned D = 257 among them); app contexts refuse SGD
tables; fp32 payloads only come from fast mode on f32 tables (no <double, float, E>); the LR
context refuses f64 tables.  The routed path of a world-1 communicator with
SWPS_PUSH_DISTINCT=0 reaches k_push_w2v_multi<T, double, 1> and k_push_lr_multi<double>
with runs of one source.
"""
import os

import numpy as np
import pytest
import torch

import table_model as tm
from conftest import GOLDEN, free_port, zipf_corpus

pytestmark = pytest.mark.gpu

from table_model import (LR_RATE, LR_SINGLE_N, MODES, N_SINGLE, SERVED_DIMS, SERVED_EXTRA, SERVED_FORMS, SLICE_DIMS,
                         SORT_LOGCAPS, WORLDS, context_accepts, served_case, single_case)

SEED = 11
LR_DATA = os.path.join(GOLDEN, "lr_data.txt")


def dev(a):
    """A numpy array on the GPU (uint64 keys as the int64 of the same bits)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.as_tensor(a).to("cuda")


def host(t):
    return t.cpu().numpy()


def push_form(dtype, D):
    E = 4 if dtype == "f32" else 2
    e = E if D % E == 0 else 1
    return "E%d-trips%d" % (e, (D // e + 63) // 64)


def pull_form(layout, dtype, D):
    es = 4 if dtype == "f32" else 8
    R, P = (4 * D, 2 * D) if layout == "w2v" else (2, 1)
    if P <= 4 and P * es < 16:
        return "out_t"
    return "out16" if (R * es) % 16 == 0 and (P * es) % 16 == 0 else "generic"


def table_sync(lib, t):
    from swiftmpi_amd import capi
    capi.check(capi.lib().swps_table_sync(t.h))


# ==== 2. single-source push, pull, assign and export ===========================================
PUSH_DIMS = [1, 2, 3, 4, 5, 7, 8, 127, 128, 129, 130, 255, 256, 257, 260, 300, 513]


def drive_single(lib, layout, D, dtype, rule, n, gtype=np.float64):
    case = single_case(layout, D, dtype, rule, n, gtype)
    keys, rows = case["keys"], case["rows"]
    kw = dict(dim=D, capacity=n + 7, dtype=dtype, learning_rate=LR_RATE, init="hash", seed=SEED, push_rule=rule)
    t = lib.Table(layout, **kw)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=LR_RATE, rule=rule, seed=SEED)
    dk = dev(keys)
    # pull: find-or-insert, hash init, the pull copy
    v = host(t.pull(dk))
    assert tm.same_bits(v, m.pull(keys)), "hash init differs from the model"
    assert t.size() == n
    assert tm.same_bits(host(t.pull(dk[:n // 2])), v[:n // 2])
    # assign / export: the round trip alone
    t.assign(dk, dev(rows))
    m.assign(keys, rows)
    tm.assert_rows_equal(host(t.export(dk)), rows, layout, "assigned")
    assert tm.same_bits(host(t.pull(dk)), rows[:, :m.P])
    # push a shuffled subset, twice
    pushed = np.zeros(n, dtype=bool)
    for sub, g in case["pushes"]:
        assert g.shape == (len(sub), m.P)
        t.push(dev(keys[sub]), dev(g))
        table_sync(lib, t)
        m.push(keys[sub], g)
        pushed[sub] = True
    assert pushed.any() and not pushed.all()
    out = host(t.export(dk))
    tm.assert_rows_equal(out[pushed], m.export(keys[pushed]), layout, "pushed")
    tm.assert_rows_equal(out[~pushed], rows[~pushed], layout, "not pushed")
    assert t.size() == n
    assert tm.same_bits(host(t.pull(dk)), out[:, :m.P])
    t.close()


@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
@pytest.mark.parametrize("dtype,D", [pytest.param(dt, D, id="%s-D%d-%s-pull_%s" % (dt, D, push_form(dt, D),
                                                                                  pull_form("w2v", dt, D)))
                                     for dt in ("f32", "f64") for D in PUSH_DIMS])
def test_single_source_w2v(lib, gpu, dtype, D, rule):
    """k_find_or_insert, k_init_rows, k_copy_rows_in / _out / _out_t / _out16, k_lookup and
    k_push_w2v<T, double, E> (the form is in the test id)."""
    drive_single(lib, "w2v", D, dtype, rule, N_SINGLE)


@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_single_source_lr(lib, gpu, dtype, rule):
    """k_push_lr<T> (every operation in T), k_copy_rows_out_t<T>; about 2 % of the gradients are
    exact zeros (the CPU module asserts it on these inputs)."""
    drive_single(lib, "lr", 1, dtype, rule, LR_SINGLE_N, gtype=np.float32)


PULL_FORMS = [("w2v", "f32", 1, "out_t"), ("lr", "f32", 1, "out_t"), ("lr", "f64", 1, "out_t"),
              ("w2v", "f32", 2, "out16"), ("w2v", "f32", 4, "out16"), ("w2v", "f64", 1, "out16"),
              ("w2v", "f64", 3, "out16"), ("w2v", "f32", 3, "generic"), ("w2v", "f32", 65, "generic")]


@pytest.mark.parametrize("layout,dtype,D,form", PULL_FORMS, ids=["%s-%s-D%d-%s" % c for c in PULL_FORMS])
def test_pull_forms_serve_a_rowless_key_as_zeros(lib, gpu, layout, dtype, D, form):
    """Each form of table_copy_pull with kNoRow rows in the call: a full table's overflow keys
    (as test_full_table_overflow_key_is_never_a_row builds them; the latched OOM is the call's
    answer) come back as zeros, the stored keys as their rows."""
    from swiftmpi_amd import capi
    assert pull_form(layout, dtype, D) == form
    cap, n = 4, 7
    t = lib.Table(layout, dim=D, capacity=cap, dtype=dtype, init="hash", seed=SEED)
    keys = tm.gen_keys(np.random.default_rng(5), n)
    dk = dev(keys)
    out = torch.full((n, t.pull_elems), 7.0, dtype=t.torch_dtype, device="cuda")
    torch.cuda.synchronize()  # the fill is done before the table's own stream writes
    rc = capi.lib().swps_pull(t.h, capi.ptr(dk), n, capi.ptr(out))
    assert rc == -1, "a pull past the capacity must report OOM"
    stored = set(t.keys().tolist())
    assert len(stored) == cap and stored <= set(keys.tolist())
    want = tm.hash_init(SEED, keys, layout, D, tm.DT[dtype])[:, :t.pull_elems]
    want[[k not in stored for k in keys.tolist()]] = 0
    assert tm.same_bits(host(out), want)
    # the same rows again through a lookup-only pull of the overflow keys: still zeros, still an error
    over = np.array([k for k in keys.tolist() if k not in stored], dtype=np.uint64)
    dover = dev(over)
    out2 = torch.full((len(over), t.pull_elems), 7.0, dtype=t.torch_dtype, device="cuda")
    torch.cuda.synchronize()
    assert capi.lib().swps_pull(t.h, capi.ptr(dover), len(over), capi.ptr(out2)) == -1
    assert not host(out2).any()
    t.close()


# ==== 3. multi-source push through the served path ==============================================

@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return zipf_corpus(str(tmp_path_factory.mktemp("table_model") / "tiny.txt"), 40, 30, 1)


class Served:
    """A sharded app context driven with synthetic keys: swps_<app>_shard(h, 0, world, frag) needs
    no communicator; the step slot stays -1, so no cached sort is taken."""

    def __init__(self, lib, layout, dtype, D, world, mode="fast", corpus=None, capacity=None):
        from swiftmpi_amd import capi
        self.capi, self.layout, self.world = capi, layout, world
        self.t = lib.Table(layout, dim=D, capacity=capacity or 256, dtype=dtype, learning_rate=LR_RATE, init="hash",
                           seed=SEED)
        if layout == "w2v":
            self.pfx, self.width = "w2v", 2 * D
            self.ctx = lib.Word2Vec(self.t, init="table", fp64_intermediates=(mode != "fast"), unigram_size=1000,
                                    minibatch=10)
            self.ctx.load_text(corpus)
            frag = 1000
        else:
            self.pfx, self.width = "lr", 1
            self.ctx = lib.LR(self.t, minibatch=200, init_ref=False)
            self.ctx.load_text(LR_DATA)
            frag = 2000
        capi.check(self._fn("shard")(self.ctx.h, 0, world, frag))
        self.pending = None

    def _fn(self, name):
        return getattr(self.capi.lib(), "swps_%s_%s" % (self.pfx, name))

    def pull(self, dkeys, counts, insert):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        assert len(counts) == self.world and int(counts.sum()) == dkeys.numel()
        out = torch.empty((dkeys.numel(), self.width), dtype=self.t.torch_dtype, device="cuda")
        self.capi.check(self._fn("serve_pull")(self.ctx.h, self.capi.ptr(dkeys), self.capi.ptr(counts), insert,
                                               self.capi.ptr(out)))
        self.sync()
        return host(out)

    def push(self, dkeys, dgrads, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        assert len(counts) == self.world and int(counts.sum()) == dkeys.numel() == dgrads.shape[0]
        self.pending = (dkeys, dgrads)  # the push reads them until the next sync
        self.capi.check(self._fn("serve_push")(self.ctx.h, self.capi.ptr(dkeys), self.capi.ptr(dgrads),
                                               self.capi.ptr(counts)))

    def sync(self):
        try:
            self.capi.check(self.capi.lib().swps_table_sync(self.t.h))
        finally:
            self.pending = None

    def close(self):
        self.ctx.close()
        self.t.close()


def run_served(lib, case, mode="fast", corpus=None):
    """serve_pull(insert) -> hash init; assign; serve_pull and serve_push per push; export: all against
    the model's push_sources."""
    layout, D, dtype = case["layout"], case["D"], case["dtype"]
    keys, skeys, counts = case["keys"], case["skeys"], case["counts"]
    s = Served(lib, layout, dtype, D, case["world"], mode, corpus, capacity=len(keys) + 3)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=LR_RATE, seed=SEED)
    dk, dsk = dev(keys), dev(skeys)
    assert tm.same_bits(s.pull(dsk, counts, 1), m.pull(skeys)), "served hash init differs from the model"
    assert s.t.size() == m.size() == len(set(skeys.tolist()))
    s.t.assign(dk, dev(case["rows"]))
    m.assign(keys, case["rows"])
    for g in case["grads"]:
        assert tm.same_bits(s.pull(dsk, counts, 0), m.export(skeys)[:, :m.P])  # LR: a push follows its pull
        s.push(dsk, dev(g), counts)
        m.push_sources(skeys, g, counts)
    s.sync()
    out = host(s.t.export(dk))
    touched = np.isin(keys, skeys)
    assert touched.sum() == len(keys) - SERVED_EXTRA
    tm.assert_rows_equal(out[touched], m.export(keys[touched]), layout, "served")
    tm.assert_rows_equal(out[~touched], case["rows"][~touched], layout, "untouched")
    assert s.t.size() == len(keys)
    s.close()


def run_served_w2v(lib, corpus, mode, D, worlds=WORLDS, single=True):
    dtype, gtype = MODES[mode]
    for world in worlds:
        run_served(lib, served_case("w2v", dtype, gtype, D, world), mode, corpus)
    if single:
        run_served(lib, served_case("w2v", dtype, gtype, D, 3, single=True), mode, corpus)


SERVED_CASES = [pytest.param(mode, D, id="%s-D%d" % (mode, D)) for mode in MODES for D in SERVED_DIMS
                if context_accepts(MODES[mode][0], D)]
REFUSED_CASES = [pytest.param(mode, D, id="%s-D%d" % (mode, D)) for mode in MODES for D in SERVED_DIMS
                 if not context_accepts(MODES[mode][0], D)]


@pytest.mark.parametrize("mode,D", SERVED_CASES)
def test_served_w2v(lib, gpu, corpus, mode, D):
    """k_lookup, k_push_keys, the sort and k_push_w2v_multi_t<1|2|3> (fast mode at the slice
    dimensions, SERVED_FORMS) or k_push_w2v_multi<T, G, E>, at worlds 2, 3 and 5; one source of
    three takes the distinct path: k_push_w2v_multi_t<NCH> without pos_s, or k_push_w2v<T, G, E>
    (G = float in fast mode)."""
    run_served_w2v(lib, corpus, mode, D)


@pytest.mark.parametrize("mode,D", REFUSED_CASES)
def test_context_refuses_dim(lib, gpu, mode, D):
    """The W2V context refuses rows that are no multiple of 16 bytes and more than 4 chunks of 64
    lanes: these dimensions of the issue's list (the slice kernel's misaligned D = 257 among
    them) never reach a served push, and no push kernel runs here."""
    dtype, _ = MODES[mode]
    assert "refused" in SERVED_FORMS[D] or dtype == "f64"
    t = lib.Table("w2v", dim=D, capacity=16, dtype=dtype)
    with pytest.raises(lib.SwpsError) as e:
        lib.Word2Vec(t, init="table", fp64_intermediates=(mode != "fast"), unigram_size=1000)
    assert e.value.code == -7
    t.close()


@pytest.mark.parametrize("D", SLICE_DIMS, ids=["D%d" % D for D in SLICE_DIMS])
def test_served_w2v_slice_push_off(lib, gpu, corpus, monkeypatch, D):
    """SWPS_SLICE_PUSH=0 (read when the table is created): the slice dimensions through
    k_push_w2v_multi<float, float, 4> (one source: k_push_w2v<float, float, 4>); both settings
    equal the model, hence each other."""
    monkeypatch.setenv("SWPS_SLICE_PUSH", "0")
    run_served_w2v(lib, corpus, "fast", D)


@pytest.mark.parametrize("mode,D", [(mode, D) for mode in MODES for D in SERVED_DIMS + [130]
                                    if context_accepts(MODES[mode][0], D)])
def test_served_w2v_single_source_distinct_off(lib, gpu, corpus, monkeypatch, mode, D):
    """SWPS_PUSH_DISTINCT=0: one source through the grouping sort and the multi kernels (runs of
    one)."""
    monkeypatch.setenv("SWPS_PUSH_DISTINCT", "0")
    run_served_w2v(lib, corpus, mode, D, worlds=[], single=True)


@pytest.mark.parametrize("world", WORLDS + ["single", "single-distinct-off"])
def test_served_lr(lib, gpu, monkeypatch, world):
    """k_push_lr_multi<float>; one source: k_push_lr<float>."""
    if world == "single-distinct-off":
        monkeypatch.setenv("SWPS_PUSH_DISTINCT", "0")
    if isinstance(world, str):
        run_served(lib, served_case("lr", "f32", "f32", 1, 3, single=True))
    else:
        run_served(lib, served_case("lr", "f32", "f32", 1, world))


def test_lr_context_refuses_f64_tables(lib, gpu):
    """So k_push_lr_multi<double> is reached by the routed path only (below)."""
    t = lib.Table("lr", capacity=16, dtype="f64")
    with pytest.raises(lib.SwpsError) as e:
        lib.LR(t, init_ref=False)
    assert e.value.code == -7
    t.close()


@pytest.mark.parametrize("layout,mode,D", [("w2v", "fast", 300), ("w2v", "fast", 8), ("w2v", "parity", 516),
                                           ("w2v", "f64", 130), ("lr", "fast", 1)])
def test_served_push_with_an_unknown_key(lib, gpu, corpus, layout, mode, D):
    """A key the table lacks in the middle source's list: its row is `capacity` for the sort
    (last, skipped), the next sync reports BADKEY, every other row equals the model."""
    dtype, gtype = MODES[mode]
    case = served_case(layout, dtype, gtype, D, 3)
    keys, counts = case["keys"], case["counts"].copy()
    at = int(counts[0] + counts[1] // 2)
    unknown = np.uint64(0x0123456789abcdef)
    assert unknown not in keys
    skeys = np.insert(case["skeys"], at, unknown)
    g = case["grads"][0]
    g = np.insert(g, at, np.full(g.shape[1], 0.25, dtype=g.dtype), axis=0)
    counts[1] += 1
    s = Served(lib, layout, dtype, D, 3, mode, corpus, capacity=len(keys) + 3)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=LR_RATE, seed=SEED)
    s.t.assign(dev(keys), dev(case["rows"]))
    m.assign(keys, case["rows"])
    dsk = dev(skeys)
    if layout == "lr":  # a push follows the pull of the same keys; its lookup latches the miss too
        with pytest.raises(lib.SwpsError) as e:
            s.pull(dsk, counts, 0)
        assert e.value.code == -2
    s.push(dsk, dev(g), counts)
    with pytest.raises(lib.SwpsError) as e:
        s.sync()
    assert e.value.code == -2 and "new key should be inited" in str(e.value)
    s.sync()  # the error is reported once
    m.push_sources(case["skeys"], case["grads"][0], case["counts"])
    tm.assert_rows_equal(host(s.t.export(dev(keys))), m.export(keys), layout, "beside an unknown key")
    assert s.t.size() == len(keys)
    s.close()


# ---- the sort's digit configurations (sort_pairs: bits = bit width of `capacity`) --------------
def lr_step_arrays(w, g2, idx, grads, lr, fudge):
    """k_push_lr's AdaGrad step on state arrays, for one source (idx distinct)."""
    m = grads.astype(np.float32)
    n2 = g2[idx] + m * m
    g2[idx] = n2
    w[idx] = w[idx] + (lr * m) / np.sqrt(n2 + fudge)


SORT_DIGITS = ["11 bits: 8-bit digits", "18 bits: 9-bit digits", "20 bits: 10-bit digits", "22 bits: 8-bit digits"]


@pytest.mark.parametrize("logcap,digits", list(zip(SORT_LOGCAPS, SORT_DIGITS)),
                         ids=["cap2^%d" % c for c in SORT_LOGCAPS])
def test_sort_configurations_on_full_lr_tables(lib, gpu, logcap, digits):
    """An LR f32 table filled to exactly `capacity` in one served pull, then three overlapping
    sources whose keys include the lowest and the highest row, against the vectorised model."""
    cap = 1 << logcap
    rng = np.random.default_rng([4, logcap])
    keys = tm.gen_keys(rng, cap)
    s = Served(lib, "lr", "f32", 1, 3, capacity=cap)
    dk = dev(keys)
    fill = np.array([cap, 0, 0], dtype=np.uint64)
    v = s.pull(dk, fill, 1)[:, 0]  # sync: no error
    assert s.t.size() == cap
    w = tm.unit_hash(SEED, keys, np.zeros(1, dtype=np.uint64))
    assert tm.same_bits(v, w)
    assert tm.same_bits(s.pull(dk, fill, 1)[:, 0], v) and tm.same_bits(s.pull(dk, fill, 0)[:, 0], v)
    assert s.t.size() == cap
    row_key = s.t.keys()
    assert len(row_key) == cap and np.array_equal(np.sort(row_key), np.sort(keys))
    order = np.argsort(keys)
    ends = order[np.searchsorted(keys[order], row_key[[0, cap - 1]])]  # positions of rows 0 and cap - 1
    per = tm.sort_case_per(logcap)
    rest = np.setdiff1d(np.arange(cap), ends)
    src = []
    for r in range(3):
        pick = rng.choice(rest, per - 2, replace=False)
        src.append(np.concatenate([ends, pick])[rng.permutation(per)])
    idx = np.concatenate(src)
    counts = np.array([len(x) for x in src], dtype=np.uint64)
    assert (np.bincount(idx, minlength=cap) == 3).sum() >= 2
    g = tm.sort_case_grads(logcap)  # zeros included (asserted in the CPU module)
    assert len(g) == len(idx)
    g2 = np.zeros(cap, dtype=np.float32)
    lr, fudge = tm.cfg_consts(LR_RATE, 1e-6)
    dsk = dev(keys[idx])
    assert tm.same_bits(s.pull(dsk, counts, 0)[:, 0], w[idx])
    s.push(dsk, dev(g), counts)
    s.sync()
    off = 0
    for x in src:
        lr_step_arrays(w, g2, x, g[off:off + len(x), 0], lr, fudge)
        off += len(x)
    out = host(s.t.export(dk))
    tm.assert_rows_equal(out, np.stack([w, g2], axis=1), "lr", digits)
    assert s.t.size() == cap
    s.close()


# ---- the routed path of a world-1 communicator: E = 1 and LR f64 in the multi form ---------------
@pytest.mark.parametrize("layout,dtype,D", [("w2v", "f32", 5), ("w2v", "f32", 65), ("w2v", "f64", 3),
                                            ("lr", "f64", 1)])
def test_routed_world1_multi_form(lib, gpu, monkeypatch, layout, dtype, D):
    """SWPS_PUSH_DISTINCT=0 on a routed table: every push goes through k_push_keys, the sort and
    k_push_w2v_multi<T, double, E> (E = 1 at the odd D, which no app context accepts) or
    k_push_lr_multi<T> (T = double: the LR context refuses such tables), with runs of one."""
    from swiftmpi_amd.comm import Comm
    monkeypatch.setenv("SWPS_PUSH_DISTINCT", "0")
    n = 150 if layout == "w2v" else 2000
    rng = np.random.default_rng([5, layout == "lr", dtype == "f64", D])
    keys = tm.gen_keys(rng, n)
    comm = Comm.rccl(0, 1, port=free_port())
    t = lib.Table(layout, dim=D, capacity=n + 5, dtype=dtype, learning_rate=LR_RATE, init="hash", seed=SEED)
    t.route(comm, frag_num=1000)
    m = tm.TableModel(layout, dim=D, dtype=dtype, learning_rate=LR_RATE, seed=SEED)
    dk = dev(keys)
    assert tm.same_bits(host(t.pull(dk)), m.pull(keys))
    G = np.float64 if layout == "w2v" else np.float32
    for _ in range(3):  # the first push starts from zero sums, the others from the sums it left
        sub = rng.permutation(n)[:(3 * n) // 4]
        g = tm.gen_grads(rng, len(sub), m.P, G)
        t.push(dev(keys[sub]), dev(g))
        m.push(keys[sub], g)
    t.barrier()
    t.finish()
    tm.assert_rows_equal(host(t.export(dk)), m.export(keys), layout, "routed")
    t.close()
    comm.close()


# ==== 4. keys, capacities, hash init ===========================================================
def test_empty_key_is_refused_and_the_call_s_other_keys_work(lib, gpu):
    from swiftmpi_amd import capi
    D = 4
    t = lib.Table("w2v", dim=D, capacity=16, dtype="f32", init="hash", seed=SEED)
    keys = np.array([5, 0, 2 ** 64 - 1, 2 ** 64 - 2, 77], dtype=np.uint64)
    with pytest.raises(lib.SwpsError) as e:
        t.pull(dev(keys))
    assert e.value.code == -2 and "empty key" in str(e.value)
    good = np.delete(keys, 2)
    assert t.size() == 4 and sorted(t.keys().tolist()) == sorted(good.tolist())
    want = tm.hash_init(SEED, keys, "w2v", D, np.float32)[:, :2 * D]
    want[2] = 0  # the empty key has no row
    dk = dev(keys)
    out = torch.full((5, 2 * D), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # the fill is done before the table's own stream writes
    assert capi.lib().swps_pull(t.h, capi.ptr(dk), 5, capi.ptr(out)) == -2
    assert tm.same_bits(host(out), want)
    # keys 0 and 2^64 - 2 are ordinary keys: pull, push and export work, nothing is latched
    assert tm.same_bits(host(t.pull(dev(good))), want[[0, 1, 3, 4]])
    m = tm.TableModel("w2v", dim=D, dtype="f32", learning_rate=0.7, seed=SEED)
    m.pull(good)
    g = tm.gen_grads(np.random.default_rng(6), 4, 2 * D, np.float64)
    t.push(dev(good), dev(g))
    table_sync(lib, t)
    m.push(good, g)
    tm.assert_rows_equal(host(t.export(dev(good))), m.export(good))
    # a push of the empty key is an unknown key
    with pytest.raises(lib.SwpsError) as e:
        t.push(dev(keys[2:3]), dev(g[:1]))
    assert e.value.code == -2
    t.close()


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_small_capacities_fill_exactly(lib, gpu, cap):
    t = lib.Table("lr", capacity=cap, dtype="f32", init="hash", seed=SEED)
    keys = tm.gen_keys(np.random.default_rng(cap), cap + 1)
    v = host(t.pull(dev(keys[:cap])))
    assert t.size() == cap
    assert tm.same_bits(v, tm.hash_init(SEED, keys[:cap], "lr", 1, np.float32)[:, :1])
    with pytest.raises(lib.SwpsError) as e:
        t.pull(dev(keys[cap:]))
    assert e.value.code == -1
    assert t.size() == cap and tm.same_bits(host(t.pull(dev(keys[:cap]))), v)
    t.close()


@pytest.mark.parametrize("layout,dtype,D", [("w2v", "f32", 17), ("w2v", "f64", 17), ("w2v", "f32", 300),
                                            ("w2v", "f64", 300), ("lr", "f32", 1), ("lr", "f64", 1)])
def test_hash_init_equals_the_model_in_any_insert_order(lib, gpu, layout, dtype, D):
    """k_init_rows on rows wider than one wave, whole rows (export: the sums start at zero), and
    the same keys inserted in two orders into two tables."""
    n = 200
    rng = np.random.default_rng([6, D])
    keys = tm.gen_keys(rng, n)
    want = tm.hash_init(SEED, keys, layout, D, tm.DT[dtype])
    kw = dict(dim=D, capacity=n, dtype=dtype, init="hash", seed=SEED)
    a, b = lib.Table(layout, **kw), lib.Table(layout, **kw)
    perm = rng.permutation(n)
    a.pull(dev(keys))
    b.pull(dev(keys[perm][:n // 2]))
    b.pull(dev(keys[perm][n // 2:][::-1]))
    for t in (a, b):
        assert t.size() == n
        tm.assert_rows_equal(host(t.export(dev(keys))), want, layout, "hash init")
    other = lib.Table(layout, **dict(kw, seed=SEED + 1))
    assert not tm.same_bits(host(other.pull(dev(keys))), want[:, :other.pull_elems])
    for t in (a, b, other):
        t.close()
