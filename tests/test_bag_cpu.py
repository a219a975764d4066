"""CPU guard for tests/test_bag_gpu.py (no GPU): the NumPy model of the pooled calls
(tests/bag_model.py) and the fixed inputs of the GPU tests tell a wrong order or a wrong operand
from the right one, and the library exports and guards the four new calls.

What each doctoring can show, by arithmetic (X = float32(1e16); "unweighted" because a random
weight per position destroys the hand-set column 0):
  onechain    one chain per bag instead of chunks of 128 positions: every unweighted case (the
              CHUNKY bag's column 0 gives 0 instead of 2; under the mean 0 instead of 2 / 257).
  descending  positions (and chunks) in descending order: every unweighted case (the MAG bag gives
              0 instead of 1).
  zero        chains started from 0.0: every unweighted case (the NEGZ bag of -0.0 values gives
              +0.0 instead of -0.0).
  mulmean     mean as sum * (1 / m): mode "mean", every table (the MEAN3 bag: the two fp64 quotients
              differ, and they straddle an fp32 rounding boundary, so the cast to fp32 keeps the
              difference).  Under "sum" the variant IS the true model (asserted equal).
  tacc        accumulation in the table dtype: fp32 tables (a bag of 127 random fp32 values summed
              in fp32 against fp64-then-one-cast differs in some element with near certainty; the
              long bags make it certain on these inputs).  On an fp64 table it IS the true model.
  padcount    padding counted in m_b: mode "mean" (the pad_head / pad_mid / pad_tail bags divide by
              3 instead of 2, the hole bag by 300 instead of 172).  Under "sum": the true model.
  w32         the weight applied in fp32: weighted calls (the W32 bag: (1 + 2^-23) * (1 + 2^-24) is
              2^-47 above the fp32 midpoint and casts to 1 + 2^-22; float32(1 + 2^-24) is 1.0 and
              leaves 1 + 2^-23; the fp64 results differ likewise).
  keymean     (backward) the divisor applied to a key's sum instead of to each term: mode "mean",
              once a key sits in bags of different member counts, which the random keys of the
              case do (40 keys over bags of 1 .. 3000 members).
"""
import ctypes

import numpy as np
import pytest

import bag_model as bm
import dup_model as dm
import table_model as tm

CASES = [("w2v", D, dt) for D in (4, 5, 6, 100, 300) for dt in ("f32", "f64")] + [("lr", 1, "f32"), ("lr", 1, "f64")]
SMALL = [c for c in CASES if c[1] <= 6]


def seq(v):
    acc = v[0].copy()
    for x in v[1:]:
        acc = acc + x
    return acc


def test_pool_rule_by_hand():
    rng = np.random.default_rng(1)
    v = rng.normal(0, 1, (400, 2))
    all_in = np.ones(400, dtype=bool)
    # one bag of 100: the plain left-to-right sum; 129 = (chain of 128) + the last
    assert tm.same_bits(bm.pool(v[:100], all_in[:100], [0, 100]), seq(v[:100])[None])
    assert tm.same_bits(bm.pool(v[:129], all_in[:129], [0, 129]), (seq(v[:128]) + v[128])[None])
    # chunks are cut by POSITION from the bag's start, not from position 0 of the call
    got = bm.pool(v[:300], all_in[:300], [0, 43, 300])
    assert tm.same_bits(got[0], seq(v[:43]))
    assert tm.same_bits(got[1], (seq(v[43:171]) + seq(v[171:299])) + v[299])
    # padding is no member: it is skipped in the chain, it does not move the chunk borders and it
    # does not count in the mean; a chunk of only padding is skipped
    mem = all_in[:300].copy()
    mem[0] = mem[5] = False
    mem[128:256] = False
    want = seq(np.concatenate([v[1:5], v[6:128]])) + seq(v[256:300])
    assert tm.same_bits(bm.pool(v[:300], mem, [0, 300])[0], want)
    assert tm.same_bits(bm.pool(v[:300], mem, [0, 300], mode="mean")[0], want / np.float64(300 - 130))
    # empty bags and a bag of only padding are +0.0, in "mean" too
    z = bm.pool(v[:3], np.array([False] * 3), [0, 0, 3, 3], mode="mean")
    assert tm.same_bits(z, np.zeros((3, 2)))
    # weights: one multiply per term, the chain from the first product
    w = rng.normal(0, 1, 3)
    assert tm.same_bits(bm.pool(v[:3], all_in[:3], [0, 3], w)[0], (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2])
    # fp32 values: accumulated in fp64, cast once
    f = v[:50].astype(np.float32)
    assert tm.same_bits(bm.pool(f, all_in[:50], [0, 50])[0], seq(f.astype(np.float64)).astype(np.float32))
    assert tm.same_bits(bm.pool(f, all_in[:50], [0, 50], mode="mean")[0],
                        (seq(f.astype(np.float64)) / np.float64(50)).astype(np.float32))
    # a key twice in a bag counts twice; -0.0 stays -0.0
    assert tm.same_bits(bm.pool(np.full((4, 1), -0.0), all_in[:4], [0, 4]), np.array([[-0.0]]))


def test_expand_rule_by_hand():
    e = int(bm.EMPTY)
    keys = np.array([7, e, 7, 9, 9, 9], dtype=np.uint64)
    off = [0, 3, 3, 6]
    G = np.array([[1.0, 2.0], [5.0, 5.0], [3.0, 7.0]])
    t = bm.expand(G, keys, off)
    assert tm.same_bits(t[[0, 2, 3]], np.array([[1.0, 2.0], [1.0, 2.0], [3.0, 7.0]]))
    t = bm.expand(G, keys, off, mode="mean")  # m = 2 (padding is no member), 0, 3
    assert tm.same_bits(t[[0, 2, 5]], np.array([[0.5, 1.0], [0.5, 1.0], [1.0, 7.0 / 3.0]]))
    w = np.array([2.0, 9.0, 0.5, 1.0, 1.0, -1.0])
    t = bm.expand(G, keys, off, w)
    assert tm.same_bits(t[[0, 2, 5]], np.array([[2.0, 4.0], [0.5, 1.0], [-3.0, -7.0]]))
    # the backward is push_dup of that matrix: key 7 gets (1 + 1), key 9 gets ((3 + 3) + 3)
    m = tm.TableModel("w2v", 1, "f64", tm.LR_RATE, rule="sgd")
    m.assign(np.array([7, 9], dtype=np.uint64), np.zeros((2, 4)))
    assert len(bm.push_bag(m, keys, off, G)) == 0
    lr = np.float64(np.float32(tm.LR_RATE))
    assert tm.same_bits(m.export([7, 9])[:, :2], np.array([[2.0, 4.0], [9.0, 21.0]]) * lr)


@pytest.mark.parametrize("layout,D,dtype", CASES)
def test_forward_doctors_differ(layout, D, dtype):
    case = bm.bag_case(layout, D, dtype)
    b = case["bags"]
    true = {(mode, wt): bm.forward(case, mode, wt) for mode, wt in (("sum", False), ("mean", False), ("sum", True))}
    # the hand-set devices do what the case's comment says
    s = true[("sum", False)]
    assert float(s[b["mag"], 0]) == 1.0 and float(s[b["chunky"], 0]) == 2.0
    assert np.signbit(s[b["negz"], case["zcol"]]) and s[b["negz"], case["zcol"]] == 0
    for e in ("empty0", "empty1", "empty2", "empty3", "empty4", "only_pad"):
        assert tm.same_bits(s[b[e]], np.zeros(case["P"], dtype=s.dtype))
        assert tm.same_bits(true[("mean", False)][b[e]], np.zeros(case["P"], dtype=s.dtype))
    for doctor in ("onechain", "descending", "zero"):
        for mode in ("sum", "mean"):
            assert not tm.same_bits(bm.forward(case, mode, False, doctor), true[(mode, False)]), (doctor, mode)
    assert tm.same_bits(bm.forward(case, "sum", False, "mulmean"), s)
    assert not tm.same_bits(bm.forward(case, "mean", False, "mulmean"), true[("mean", False)])
    assert tm.same_bits(bm.forward(case, "sum", False, "padcount"), s)
    assert not tm.same_bits(bm.forward(case, "mean", False, "padcount"), true[("mean", False)])
    assert not tm.same_bits(bm.forward(case, "sum", True, "w32"), true[("sum", True)])
    for key in true:
        t = bm.forward(case, key[0], key[1], "tacc")
        assert tm.same_bits(t, true[key]) == (dtype == "f64"), key


@pytest.mark.parametrize("layout,D,dtype", SMALL)
@pytest.mark.parametrize("rule", ["adagrad", "sgd"])
def test_backward_keymean_differs_and_equals_push_dup(layout, D, dtype, rule):
    case = bm.bag_case(layout, D, dtype)
    gtype = "f32" if layout == "lr" else "f64"
    true = bm.backward(case, gtype, rule, "mean", False, -1.0)
    assert not tm.same_bits(bm.backward(case, gtype, rule, "mean", False, -1.0, "keymean"), true)
    assert tm.same_bits(bm.backward(case, gtype, rule, "sum", False, -1.0, "keymean"),
                        bm.backward(case, gtype, rule, "sum", False, -1.0))
    # the stated consequence: push_bag is push_dup of the expanded fp64 matrix
    m = bm.case_model(case, rule)
    for G in bm.bag_grads(case, gtype):
        dm.push_dup(m, case["ids"], bm.expand(G, case["ids"], case["offsets"], None, "mean"), "sum", -1.0)
    assert tm.same_bits(m.export(case["keys"]), true)


NEW_SYMBOLS = ["swps_lookup_bag", "swps_push_bag", "swps_lookup_bag_h", "swps_push_bag_h"]
E_CFG, E_UNSUPPORTED = -5, -7


def test_library_exports_the_calls(lib):
    from swiftmpi_amd import capi
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.PROTOS
        assert getattr(L, name) is not None
    assert (capi.BAG_SUM, capi.BAG_MEAN) == (0, 1)
    import swiftmpi_amd
    from swiftmpi_amd import nn
    assert callable(swiftmpi_amd.Table.lookup_bag) and callable(swiftmpi_amd.Table.push_bag)
    assert "SparseEmbeddingBag" in nn.__all__


def test_bad_arguments_are_refused_without_a_device(lib):
    """Every refusal that precedes the first device call, with a null table or a zeroed block that
    stands in for one (nothing but its cfg.layout is read)."""
    from swiftmpi_amd import capi
    L = capi.lib()
    buf = (ctypes.c_uint64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    S, M, F32, F64 = capi.BAG_SUM, capi.BAG_MEAN, capi.F32, capi.F64
    block = ctypes.create_string_buffer(1 << 16)
    fake = ctypes.cast(block, ctypes.c_void_p)

    def calls(t, keys=p, n=4, off=p, nb=2, w=None, mode=S, insert=1, io=p, gd=F32):
        return [L.swps_lookup_bag(t, keys, n, off, nb, w, mode, insert, io, None),
                L.swps_push_bag(t, keys, n, off, nb, w, mode, io, gd, 1.0, None),
                L.swps_lookup_bag_h(t, keys, n, off, nb, w, mode, insert, io),
                L.swps_push_bag_h(t, keys, n, off, nb, w, mode, io, 1.0)]

    assert calls(None) == [E_CFG] * 4  # a null table
    assert calls(fake, keys=None) == [E_CFG] * 4  # null pointers
    assert calls(fake, off=None) == [E_CFG] * 4
    assert calls(fake, io=None) == [E_CFG] * 4
    assert b"null" in L.swps_last_error()
    assert calls(None, mode=2) == [E_CFG] * 4
    assert calls(fake, mode=2) == [E_CFG] * 4
    assert b"mode" in L.swps_last_error()
    assert L.swps_lookup_bag(fake, p, 4, p, 2, None, S, 2, p, None) == E_CFG
    assert b"insert" in L.swps_last_error()
    assert L.swps_lookup_bag_h(fake, p, 4, p, 2, None, S, 2, p) == E_CFG
    assert L.swps_push_bag(fake, p, 4, p, 2, None, S, p, 7, 1.0, None) == E_CFG
    assert b"gdtype" in L.swps_last_error()
    assert calls(fake, w=p, mode=M) == [E_CFG] * 4  # weights with the mean, as torch refuses it
    assert b"weights" in L.swps_last_error()
    # an LR table takes fp32 bag gradients
    ctypes.cast(block, ctypes.POINTER(capi.TableCfg)).contents.layout = capi.LAYOUT_LR
    assert L.swps_push_bag(fake, p, 4, p, 2, None, S, p, F64, 1.0, None) == E_CFG
    assert b"LR" in L.swps_last_error()
    ctypes.cast(block, ctypes.POINTER(capi.TableCfg)).contents.layout = capi.LAYOUT_W2V
    # positions and bag indices are 32-bit
    big = 1 << 32
    assert calls(fake, n=big) == [E_UNSUPPORTED] * 4
    assert calls(fake, nb=big) == [E_UNSUPPORTED] * 4
    # keys without bags
    assert calls(fake, nb=0) == [E_CFG] * 4
    assert b"nbags" in L.swps_last_error()
