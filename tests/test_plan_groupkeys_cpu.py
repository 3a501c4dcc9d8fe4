"""The arithmetic of the packed two-column group code (engine_abi.h
gg_plan_desc.group_cols), pinned through gg_engine_plan_group_bits: a
pure host function, so none of this needs a GPU or an Engine.

b = bit_length(max - min + 1): the column's values plus the NULL code;
a pair is accepted iff b0 + b1 <= 62."""
import ctypes

OK, ENOTSUP = 0, 5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NARROW = (-5, -5)             # 1 bit: never what tips a pair over


def bits(r0, r1):
    from greengage_amd import plan_group_bits
    return plan_group_bits([r0[0], r1[0]], [r0[1], r1[1]])


def test_budget_edge():
    r = (0, (1 << 31) - 2)
    assert bits(r, r) == (OK, (31, 31))
    assert bits((0, (1 << 31) - 1), r) == (ENOTSUP, (32, 31))
    assert bits(r, (0, (1 << 31) - 1)) == (ENOTSUP, (31, 32))


def test_single_value_takes_one_bit():
    assert bits(NARROW, NARROW) == (OK, (1, 1))


def test_null_code_counts():
    # 256 values plus the NULL code: 9 bits, not 8
    assert bits((0, 255), NARROW) == (OK, (9, 1))
    assert bits((0, 254), NARROW) == (OK, (8, 1))


def test_full_range_does_not_overflow():
    assert bits((I64_MIN + 2, I64_MAX), NARROW) == (ENOTSUP, (64, 1))
    assert bits(NARROW, (I64_MIN, I64_MAX)) == (ENOTSUP, (1, 65))
    assert bits((-1, I64_MAX), NARROW)[0] == ENOTSUP


def test_wide_values_narrow_range():
    lo = -(1 << 45)
    assert bits((lo, lo + 999), NARROW) == (OK, (10, 1))
    assert bits((lo, lo + 1023), (1 << 50, (1 << 50) + 1999)) == \
        (OK, (11, 11))


def test_empty_column_takes_one_bit():
    assert bits((I64_MAX, I64_MIN), (0, 255)) == (OK, (1, 9))


def test_plan_desc_layout_unchanged():
    from greengage_amd import engine as ge
    d = ge._PlanDesc()
    assert ctypes.sizeof(d) == ge.lib().gg_engine_plan_desc_size()
    assert d.ngroup == 0 and list(d.group_src) == [0, 0]
