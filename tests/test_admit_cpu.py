"""Admission by count without a device: the NumPy model of
tests/admit_model.py has the properties the rule promises, the fixed inputs of
tests/test_admit_gpu.py exercise both the exact rule (no false admit in the wide sketch) and the
collisions (many in the 64-cell one) and tell the two-pass rule from a per-key one, and the
argument checks of swps_table_set_admission / Table.set_admission that come before any device call."""
import functools

import numpy as np
import pytest

import admit_model as am
import dup_model as dm
import table_model as tm

E_CFG = -5


@functools.lru_cache(maxsize=None)
def the_case(nu, min_count):
    return am.stream_case(nu, min_count)


@functools.lru_cache(maxsize=None)
def the_run(nu, min_count, width, doctor=None):
    return am.run_stream(the_case(nu, min_count), min_count, width, doctor=doctor)


def test_fmix64_is_the_library_s(lib):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 2 ** 64 - 1, 50, dtype=np.uint64), np.array([0, 1, 2 ** 64 - 1], dtype=np.uint64)])
    assert [int(v) for v in am.fmix64(x)] == [lib.fmix64(int(v)) for v in x]


def test_cell_rule_by_hand(lib):
    """cell(j, key) restated with Python integers and the library's fmix64."""
    keys = tm.gen_keys(np.random.default_rng(2), 40)
    for width in (64, 1 << 16, 1 << 30):
        cols = am.cell_cols(keys, am.SEED, width)
        for j in range(am.DEPTH):
            salt = lib.fmix64((am.SEED + j) % 2 ** 64)
            assert cols[j].tolist() == [lib.fmix64(int(k) ^ salt) & (width - 1) for k in keys]


@pytest.mark.parametrize("nu", am.NUS)
@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
@pytest.mark.parametrize("width", am.WIDTHS)
def test_no_under_admission(nu, min_count, width):
    """Every key whose clipped occurrences while absent have reached min_count holds a row: false
    admits only, never false refusals (AdmitModel.gate asserts it per key; here the end state)."""
    m, trace = the_run(nu, min_count, width)
    for k, tc in m.true_count.items():
        if tc >= min_count:
            assert k in m.table.rows
    c = m.counters()
    assert c["tested"] == c["admitted"] + c["refused"] and c["admitted"] == m.table.size()
    assert trace[-1]["counters"] == c


@pytest.mark.parametrize("nu", am.NUS)
@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
def test_wide_sketch_is_exact_on_the_gpu_inputs(nu, min_count):
    """width 2^16: no false admit, so the admitted keys are exactly those of an exact counter:
    the hot keys in the first call, the once-per-call keys in call number min_count."""
    case = the_case(nu, min_count)
    m, trace = the_run(nu, min_count, 1 << 16)
    assert m.false_admits == 0
    assert set(case["hot"].tolist()) <= set(trace[0]["admitted"].tolist())
    once = set(case["once"].tolist())
    for c, t in enumerate(trace):
        got = once & set(t["admitted"].tolist())
        assert got == (once if c == min_count - 1 else set()), c
    assert m.refused > 0


@pytest.mark.parametrize("nu", [n for n in am.NUS if n > 1])
@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
def test_narrow_sketch_collides_on_the_gpu_inputs(nu, min_count):
    m, _ = the_run(nu, min_count, 64)
    assert m.false_admits > 0


@pytest.mark.parametrize("nu", [n for n in am.NUS if n > 1])
@pytest.mark.parametrize("min_count", am.MIN_COUNTS)
def test_two_pass_rule_differs_from_per_key_rule(nu, min_count):
    """A key tested before the later keys of its call have added their counts sees smaller cells:
    on the 64-cell inputs the per-key rule admits other keys, so the GPU comparison tells them apart."""
    m, trace = the_run(nu, min_count, 64)
    p, ptrace = the_run(nu, min_count, 64, "perkey")
    assert set(m.keys().tolist()) != set(p.keys().tolist())
    assert any(not np.array_equal(a["found"], b["found"]) for a, b in zip(trace, ptrace))
    # and never the other way round: whatever the per-key rule admits in the first call, the two-pass rule admits
    assert set(ptrace[0]["admitted"].tolist()) <= set(trace[0]["admitted"].tolist())


def test_saturation_and_decay():
    m = am.AdmitModel(tm.TableModel("lr", 1, "f32", seed=am.SEED), 5, 64)
    m.cells[:] = np.uint32(2 ** 32 - 3)
    keys = tm.gen_keys(np.random.default_rng(3), 200)
    m.lookup(np.repeat(keys, 5))
    assert m.cells.max() == 2 ** 32 - 1 and m.cells.min() >= 2 ** 32 - 3
    cols = am.cell_cols(keys, am.SEED, 64)
    for j in range(am.DEPTH):
        touched = np.zeros(64, dtype=bool)
        touched[cols[j]] = True
        assert np.all(m.cells[j][touched] == 2 ** 32 - 1) and np.all(m.cells[j][~touched] == 2 ** 32 - 3)
    before = m.cells.copy()
    m.decay(1)
    assert np.array_equal(m.cells, before >> np.uint32(1))
    m.decay(32)
    assert not m.cells.any()


def test_padding_and_present_keys_are_not_counted():
    t = tm.TableModel("lr", 1, "f32", seed=am.SEED)
    held = tm.gen_keys(np.random.default_rng(4), 10)
    t.pull(held)
    m = am.AdmitModel(t, 2, 64)
    ids = np.concatenate([held, held, np.full(7, dm.EMPTY, dtype=np.uint64)])
    vals, found = m.lookup(ids)
    assert not m.cells.any() and m.counters() == dict(tested=0, admitted=0, refused=0)
    assert found.tolist() == [1] * 20 + [0] * 7 and not vals[20:].any()


def bare_table(lib):
    """A Table object that never reached the library (no device): the argument checks come first."""
    t = lib.Table.__new__(lib.Table)
    t.h = None
    return t


def test_set_admission_argument_errors(lib):
    t = bare_table(lib)
    for bad in (63, 65, 100, 0, (1 << 30) + 1, 1 << 31, 3 << 10, -64):
        with pytest.raises(ValueError):
            t.set_admission(2, bad)
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError):
            t.set_admission(bad, 1 << 10)
    for bad in (2.0, "2", True, [2]):
        with pytest.raises(TypeError):
            t.set_admission(bad, 1 << 10)
        with pytest.raises(TypeError):
            t.set_admission(2, bad)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            t.admission_decay(bad)
    with pytest.raises(TypeError):
        t.admission_decay(1.0)
    with pytest.raises(TypeError):
        t.admission_load(np.zeros((4, 64), dtype=np.int64))
    for bad in (np.zeros(256, dtype=np.uint32), np.zeros((3, 64), dtype=np.uint32)):
        with pytest.raises(ValueError):
            t.admission_load(bad)


def test_c_abi_refuses_before_any_device_call(lib):
    """The width check of swps_table_set_admission comes before the table is looked at; a null
    table is SWPS_E_CFG everywhere."""
    from swiftmpi_amd import capi
    L = capi.lib()
    for width in (0, 63, 96, 1 << 31):
        assert L.swps_table_set_admission(None, 2, width) == E_CFG
        assert b"power of two" in L.swps_last_error()
    assert L.swps_table_set_admission(None, 2, 1 << 10) == E_CFG and b"null" in L.swps_last_error()
    assert L.swps_table_set_admission(None, 0, 0) == E_CFG  # off needs no width, but a table
    out = np.zeros(6, dtype=np.uint64)
    assert L.swps_admission_info(None, capi.ptr(out)) == E_CFG
    assert L.swps_admission_decay(None, 1) == E_CFG
    assert L.swps_admission_decay(None, 0) == E_CFG and b"1..32" in L.swps_last_error()
    assert L.swps_admission_cells(None, None, 0, None) == E_CFG
    assert L.swps_admission_load(None, None, 0) == E_CFG
    assert capi.ADMIT_DEPTH == am.DEPTH == 4
