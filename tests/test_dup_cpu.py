"""CPU guard for tests/test_dup_gpu.py (no GPU): the NumPy model of the repeated-key calls
(tests/dup_model.py) and the fixed inputs of the GPU tests tell a wrong summation order from
the right one, and the library exports and guards the five new calls.

What each doctoring can show, by arithmetic:
  nochunk     one sequential chain instead of chunks of 128: every case (the m = 257 run's
              column 0 gives a gradient of 0 instead of 2).
  descending  positions in descending order: every case (the MAG run gives 0 instead of 1).
  zero        chains started from 0.0: every case (a run of -0.0 gradients on a -0.0 element
              gives +0.0 instead of -0.0).
  mulmean     mean as sum * (1 / m): reduce = "mean" on fp64 W2V tables and on LR tables (the m = 3
              run's column 0 is built to sit on an fp32 rounding boundary).  The two fp64 means
              differ by one fp64 ulp at most; on an fp32 W2V table the cast of the updated element
              to fp32 absorbs that except about once in 2^29 elements, so no input of this size can
              show it there and the GPU tests cannot see such a kernel change on those tables
              either.  Under reduce = "sum" the variant IS the true model (asserted equal).
"""
import ctypes

import numpy as np
import pytest

import dup_model as dm
import table_model as tm

W2V_DIMS = [4, 5, 6, 300]
CASES = [("w2v", D, dtype, gtype) for D in W2V_DIMS for dtype in ("f32", "f64") for gtype in ("f32", "f64")] + \
        [("lr", 1, dtype, "f32") for dtype in ("f32", "f64")]


def test_coalesce_model():
    e = int(dm.EMPTY)
    keys = np.array([7, 3, e, 7, 9, 3, 7, e], dtype=np.uint64)
    uniq, inv, count = dm.coalesce(keys)
    assert uniq.tolist() == [7, 3, 9] and count.tolist() == [3, 2, 1]
    assert inv.tolist() == [0, 1, 0xFFFFFFFF, 0, 2, 1, 0, 0xFFFFFFFF]
    u, first, c = np.unique(keys[keys != dm.EMPTY], return_index=True, return_counts=True)
    order = np.argsort(first)
    assert np.array_equal(uniq, u[order]) and np.array_equal(count, c[order])


def test_combine_rule_by_hand():
    """m <= 128 is the plain left-to-right sum; m = 1 passes through; 129 values are
    (chain of 128) + the last; 257 values are (c1 + c2) + c3 with every chain from its first."""
    rng = np.random.default_rng(5)
    g = rng.normal(0, 1, (300, 2))

    def seq(v):
        acc = v[0].copy()
        for x in v[1:]:
            acc = acc + x
        return acc

    assert tm.same_bits(dm.combine(g, [17]), g[17])
    assert tm.same_bits(dm.combine(g, range(100)), seq(g[:100]))
    assert tm.same_bits(dm.combine(g, range(129)), seq(g[:128]) + g[128])
    want = (seq(g[:128]) + seq(g[128:256])) + g[256]
    assert tm.same_bits(dm.combine(g, range(257)), want)
    assert tm.same_bits(dm.combine(g, range(3), "mean", -1.0), (seq(g[:3]) / np.float64(3)) * np.float64(-1.0))
    # positions are taken in ascending order however they are listed
    assert tm.same_bits(dm.combine(g, [5, 2, 9]), (g[2] + g[5]) + g[9])
    assert tm.same_bits(dm.combine(np.full((4, 1), -0.0), range(4)), np.array([-0.0]))
    assert not tm.same_bits(dm.combine(np.full((4, 1), -0.0), range(4), doctor="zero"), np.array([-0.0]))


@pytest.mark.parametrize("layout,D,dtype,gtype", CASES)
@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
def test_doctored_variants_differ(layout, D, dtype, gtype, rule):
    case = dm.push_case(layout, D, dtype, gtype)
    for reduce, scale in (("sum", 1.0), ("mean", -1.0)):
        true = dm.run_case(case, rule, reduce, scale)
        for doctor in ("nochunk", "descending", "zero"):
            assert not tm.same_bits(dm.run_case(case, rule, reduce, scale, doctor), true), (doctor, reduce)
        mul = dm.run_case(case, rule, reduce, scale, "mulmean")
        if reduce == "sum":
            assert tm.same_bits(mul, true)
        elif dtype == "f64" or layout == "lr":
            assert not tm.same_bits(mul, true)


@pytest.mark.parametrize("layout,D,dtype", [("w2v", 6, "f32"), ("w2v", 5, "f64"), ("lr", 1, "f32")])
def test_distinct_keys_equal_plain_push(layout, D, dtype):
    rng = np.random.default_rng(6)
    keys = tm.gen_keys(rng, 40)
    rows = tm.gen_rows(rng, 40, layout, D, tm.DT[dtype])
    G = np.float64 if layout == "w2v" else np.float32
    g = tm.gen_grads(rng, 40, 2 * D if layout == "w2v" else 1, G)
    a = tm.TableModel(layout, D, dtype, tm.LR_RATE)
    b = tm.TableModel(layout, D, dtype, tm.LR_RATE)
    a.assign(keys, rows)
    b.assign(keys, rows)
    order = rng.permutation(40)
    assert len(dm.push_dup(a, keys[order], g[order])) == 0
    b.push(keys[order], g[order])
    assert tm.same_bits(a.export(keys), b.export(keys))
    # padding is skipped, an unknown key is reported and the others are applied
    k2 = np.concatenate([keys[:3], [dm.EMPTY, np.uint64(12345)]]).astype(np.uint64)
    g2 = tm.gen_grads(rng, 5, g.shape[1], G)
    assert dm.push_dup(a, k2, g2).tolist() == [12345]
    b.push(keys[:3], g2[:3])
    assert tm.same_bits(a.export(keys), b.export(keys))


NEW_SYMBOLS = ["swps_coalesce", "swps_lookup", "swps_push_dup", "swps_lookup_h", "swps_push_dup_h"]


def test_library_exports_the_calls(lib):
    from swiftmpi_amd import capi
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.PROTOS
        assert getattr(L, name) is not None
    assert (capi.REDUCE_SUM, capi.REDUCE_MEAN, capi.DUP_CHUNK) == (0, 1, dm.CHUNK)


def test_bad_arguments_are_refused_without_a_device(lib):
    """Checked before any device call: a null table, reduce = 2, gdtype = 7, insert = 2."""
    from swiftmpi_amd import capi
    L = capi.lib()
    E_CFG = -5
    buf = (ctypes.c_uint64 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nu = ctypes.c_uint64()
    assert L.swps_coalesce(None, p, 4, None, None, None, ctypes.byref(nu), None) == E_CFG
    assert L.swps_lookup(None, p, 4, 1, p, None, None) == E_CFG
    assert L.swps_lookup(None, p, 4, 2, p, None, None) == E_CFG
    assert b"insert" in L.swps_last_error()
    assert L.swps_push_dup(None, p, 4, p, capi.F32, capi.REDUCE_SUM, 1.0, None) == E_CFG
    assert L.swps_push_dup(None, p, 4, p, capi.F32, 2, 1.0, None) == E_CFG
    assert b"reduce" in L.swps_last_error()
    assert L.swps_push_dup(None, p, 4, p, 7, capi.REDUCE_SUM, 1.0, None) == E_CFG
    assert b"gdtype" in L.swps_last_error()
    assert L.swps_lookup_h(None, p, 4, 1, p, None) == E_CFG
    assert L.swps_lookup_h(None, p, 4, 2, p, None) == E_CFG
    assert L.swps_push_dup_h(None, p, 4, p, capi.REDUCE_MEAN, 1.0) == E_CFG
    assert L.swps_push_dup_h(None, p, 4, p, 2, 1.0) == E_CFG
    # positions are 32-bit: n >= 2^32 is refused before the table is looked at (a zeroed block
    # stands in for one; nothing reads it)
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    E_UNSUPPORTED = -7
    big = 1 << 32
    assert L.swps_coalesce(fake, p, big, None, None, None, ctypes.byref(nu), None) == E_UNSUPPORTED
    assert L.swps_lookup(fake, p, big, 1, p, None, None) == E_UNSUPPORTED
    assert L.swps_push_dup(fake, p, big, p, capi.F32, capi.REDUCE_SUM, 1.0, None) == E_UNSUPPORTED
    assert L.swps_lookup_h(fake, p, big, 0, p, None) == E_UNSUPPORTED
    assert L.swps_push_dup_h(fake, p, big, p, capi.REDUCE_SUM, 1.0) == E_UNSUPPORTED
