"""swps_erase_plan, the compaction rule of an erase, as a host function of
libswps against tests/erase_model.py, and the argument checks of Table.erase / prune / shrink that
run before any library call: no device needed."""
import ctypes

import numpy as np
import pytest

import erase_model as em

E_CFG = -5


def c_plan(lib, dead, cap=None):
    """swps_erase_plan through ctypes -> (rc, M, moves, src, dst)."""
    from swiftmpi_amd import capi
    d = np.ascontiguousarray(np.asarray(dead, dtype=np.uint8))
    cap = len(d) if cap is None else cap
    src = np.full(max(cap, 1), 0xFFFFFFFF, dtype=np.uint32)
    dst = np.full(max(cap, 1), 0xFFFFFFFF, dtype=np.uint32)
    m, h = ctypes.c_uint64(), ctypes.c_uint64()
    rc = capi.lib().swps_erase_plan(capi.ptr(d), len(d), ctypes.byref(m), capi.ptr(src), capi.ptr(dst), cap,
                                    ctypes.byref(h))
    return rc, m.value, h.value, src, dst


def check_mask(lib, dead):
    dead = np.asarray(dead, dtype=np.uint8)
    n, nd = len(dead), int((dead != 0).sum())
    m, src, dst = em.plan(dead)
    rc, cm, ch, csrc, cdst = c_plan(lib, dead)
    assert rc == 0 and cm == m == n - nd and ch == len(src)
    assert np.array_equal(csrc[:ch], src) and np.array_equal(cdst[:ch], dst)
    assert np.all(csrc[ch:] == 0xFFFFFFFF) and np.all(cdst[ch:] == 0xFFFFFFFF)  # nothing written past the moves
    # the properties the in-place copy rests on
    assert np.all(src >= m) and np.all(dst < m)
    assert np.all(np.diff(src.astype(np.int64)) > 0) and np.all(np.diff(dst.astype(np.int64)) > 0)
    assert ch <= min(nd, m)
    assert np.all(dead[dst] != 0) and np.all(dead[src] == 0)
    # the Python wrapper, and what the rule does to a row order
    pm, psrc, pdst = lib.erase_plan(dead)
    assert pm == m and np.array_equal(psrc, src) and np.array_equal(pdst, dst)
    keys = np.arange(100, 100 + n, dtype=np.uint64)
    after = em.apply(keys, dead)
    assert len(after) == m and set(after.tolist()) == set(keys[dead == 0].tolist())
    stay = np.ones(n, dtype=bool)
    stay[dst] = False
    assert np.array_equal(after[stay[:m]], keys[:m][stay[:m]])  # every row that is no hole stays put
    return m, ch


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_random_masks(lib, n):
    rng = np.random.default_rng([15, n])
    for p in (0.1, 0.5, 0.9):
        for _ in range(4):
            check_mask(lib, rng.random(n) < p)


def test_none_dead(lib):
    for n in (0, 1, 64, 257):
        assert check_mask(lib, np.zeros(n)) == (n, 0)


def test_all_dead(lib):
    for n in (1, 2, 65, 257):
        assert check_mask(lib, np.ones(n)) == (0, 0)


def test_tail_only(lib):
    d = np.zeros(257)
    d[200:] = 1
    assert check_mask(lib, d) == (200, 0)  # the dead rows are exactly the rows past M: no move
    d = np.zeros(2)
    d[1] = 1
    assert check_mask(lib, d) == (1, 0)


def test_head_only(lib):
    d = np.zeros(257)
    d[:57] = 1
    m, h = check_mask(lib, d)
    assert (m, h) == (200, 57)
    _, src, dst = lib.erase_plan(d)
    assert np.array_equal(dst, np.arange(57)) and np.array_equal(src, np.arange(200, 257))


def test_more_dead_than_survivors(lib):
    d = np.ones(65)
    d[[3, 40, 64]] = 0
    m, h = check_mask(lib, d)
    assert m == 3 and h == 3  # rows 0..2 are dead: every survivor moves, moves = min(#dead, M) = M
    _, src, dst = lib.erase_plan(d)
    assert src.tolist() == [3, 40, 64] and dst.tolist() == [0, 1, 2]
    d[1], d[40] = 0, 1  # the survivors are rows 1, 3 and 64: row 1 is below M and stays
    assert check_mask(lib, d) == (3, 2)
    _, src, dst = lib.erase_plan(d)
    assert src.tolist() == [3, 64] and dst.tolist() == [0, 2]


def test_alternating(lib):
    for n in (64, 65):
        for first in (0, 1):
            d = (np.arange(n) + first) % 2
            m, h = check_mask(lib, d)
            assert m == n - int(d.sum()) and h == int(d[:m].sum())


def test_small_buffers_are_refused(lib):
    d = np.zeros(257, dtype=np.uint8)
    d[:57] = 1
    for cap in (0, 1, 56):
        rc, m, h, src, dst = c_plan(lib, d, cap=cap)
        assert rc == E_CFG and (m, h) == (200, 57)
        assert np.all(src == 0xFFFFFFFF) and np.all(dst == 0xFFFFFFFF)  # untouched
    rc, m, h, src, dst = c_plan(lib, d, cap=57)
    assert rc == 0 and h == 57
    # no move needed: no room needed
    assert c_plan(lib, np.zeros(9, dtype=np.uint8), cap=0)[:3] == (0, 9, 0)


def bare_table(lib):
    """A Table object that never reached the library (no device): the argument checks come first."""
    t = lib.Table.__new__(lib.Table)
    t.h = None
    return t


def test_erase_rejects_non_integer_keys(lib):
    import torch
    t = bare_table(lib)
    for bad in (np.array([1.0, 2.0]), np.array(["a"]), [0.5], np.array([True, False])):
        with pytest.raises(TypeError):
            t.erase(bad)
    for bad in (torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(TypeError):
            t.erase(bad)
    with pytest.raises(TypeError):  # a host tensor is not device keys
        t.erase(torch.zeros(3, dtype=torch.int64))


def test_prune_rejects_bad_thresholds(lib):
    t = bare_table(lib)
    for bad in (float("nan"), -1.0, -1e-30, np.float32(-2)):
        with pytest.raises(ValueError):
            t.prune(bad)
    for bad in ("0", None, [0.0], True):
        with pytest.raises(TypeError):
            t.prune(bad)


def test_shrink_rejects_negative_keys(lib):
    with pytest.raises(ValueError):
        bare_table(lib).shrink(-1)
