"""swps_grow_plan, the growth policy of a table under a ceiling, as a host
function of libswps: no device needed.

    new_capacity = capacity                      when nrows + incoming <= capacity or max == 0
                 = min(max(2 capacity, nrows + incoming), max(max, capacity))   otherwise
    new_slots    = the smallest power of two >= 2 new_capacity (swps_table_create's rule)
"""
import pytest


@pytest.fixture(scope="module")
def plan(lib):
    return lib.grow_plan


def create_slots(capacity):
    """swps_table_create: ns = 1; while (ns < 2 * capacity) ns <<= 1."""
    ns = 1
    while ns < 2 * capacity:
        ns <<= 1
    return ns


def test_no_growth_while_the_keys_fit(plan):
    assert plan(8, 1024, 5, 3)[0] == 8          # nrows + incoming == capacity
    assert plan(8, 1024, 0, 8)[0] == 8
    assert plan(8, 1024, 8, 0)[0] == 8
    assert plan(8, 1024, 0, 0)[0] == 8
    assert plan(8, 1024, 5, 4)[0] == 16         # one key more grows


def test_doubling(plan):
    assert plan(4, 1024, 3, 2) == (8, 16)
    assert plan(4, 1024, 4, 1) == (8, 16)
    assert plan(100, 10 ** 6, 100, 50) == (200, 512)
    assert plan(100, 10 ** 6, 100, 100) == (200, 512)   # nrows + incoming == 2 capacity


def test_jump_past_the_doubling(plan):
    assert plan(4, 1024, 3, 33) == (36, 128)
    assert plan(4, 1024, 0, 9) == (9, 32)
    assert plan(16, 10 ** 7, 16, 71290) == (71306, create_slots(71306))


def test_clipped_at_the_ceiling(plan):
    assert plan(8, 12, 8, 1) == (12, 32)
    assert plan(8, 16, 0, 20) == (16, 32)
    assert plan(8, 8, 8, 1) == (8, 16)          # at the ceiling: no growth, the insert overflows
    assert plan(8, 15, 8, 100) == (15, 32)
    # a ceiling below the capacity (reserve may exceed it) never shrinks the table
    assert plan(32, 16, 32, 5) == (32, 64)


def test_zero_ceiling_never_grows(plan):
    for cap, nrows, inc in [(4, 4, 1), (4, 0, 1000), (1, 1, 1), (1000, 999, 2), (8, 8, 2 ** 40)]:
        assert plan(cap, 0, nrows, inc) == (cap, create_slots(cap))


def test_huge_incoming_saturates(plan):
    assert plan(4, 1000, 3, 2 ** 64 - 1)[0] == 1000
    assert plan(4, 1000, 2 ** 63, 2 ** 63)[0] == 1000


CAPS = sorted({1, 3, 4, 5} | {2 ** k + d for k in range(1, 31) for d in (-1, 0, 1)} | {2 ** 31 + 1, 0xFFFFFFEF})


@pytest.mark.parametrize("cap", CAPS)
def test_slots_follow_the_create_rule(plan, cap):
    nc, ns = plan(cap, 0, 0, 0)
    assert nc == cap and ns == create_slots(cap)
    assert ns & (ns - 1) == 0 and ns >= 2 * nc and (ns == 1 or ns // 2 < 2 * nc)
    # grown: the slots of the NEW capacity
    ceiling = min(4 * cap + 3, 0xFFFFFFEF)
    nc, ns = plan(cap, ceiling, cap, 1)
    assert nc == min(max(2 * cap, cap + 1), ceiling)
    assert ns == create_slots(nc) and ns & (ns - 1) == 0 and ns >= 2 * nc


def test_bad_arguments(lib, plan):
    for args in [(0, 0, 0, 0), (0xFFFFFFF0, 0, 0, 0), (8, 0xFFFFFFF0, 0, 0)]:
        with pytest.raises(lib.SwpsError) as e:
            plan(*args)
        assert e.value.code == -5
