"""The Python binding's aggregate-kind constants must match the
gg_plan_aggkind enum of include/engine_abi.h (no GPU needed)."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enum_values():
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        src = f.read()
    body = re.search(r"typedef enum gg_plan_aggkind\s*\{(.*?)\}\s*"
                     r"gg_plan_aggkind;", src, re.S).group(1)
    return {m.group(1): int(m.group(2))
            for m in re.finditer(r"(GG_AGG_\w+)\s*=\s*(\d+)", body)}


def test_aggkind_constants_match_header():
    from greengage_amd import engine as ge
    vals = _enum_values()
    assert vals == {"GG_AGG_COUNT_STAR": 0, "GG_AGG_COUNT_COL": 1,
                    "GG_AGG_SUM": 2, "GG_AGG_MIN": 3, "GG_AGG_MAX": 4,
                    "GG_AGG_AVG": 5}
    assert ge.AGG_MIN == vals["GG_AGG_MIN"]
    assert ge.AGG_MAX == vals["GG_AGG_MAX"]
    assert ge.AGG_AVG == vals["GG_AGG_AVG"]
    assert (ge.AGG_COUNT_STAR, ge.AGG_COUNT_COL, ge.AGG_SUM) == (0, 1, 2)


def test_library_exports_compile_plan():
    from greengage_amd import engine as ge
    fn = ge.lib().gg_engine_compile_plan
    assert ctypes.cast(fn, ctypes.c_void_p).value
