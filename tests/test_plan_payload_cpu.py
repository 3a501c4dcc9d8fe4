"""The Python binding's mirror of the extended plan descriptor must
match include/engine_abi.h: the join-kind constants against the
gg_plan_joinkind enum, and the ctypes layout of gg_plan_desc against
the size the built library reports (no GPU needed)."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enum_values():
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        src = f.read()
    body = re.search(r"typedef enum gg_plan_joinkind\s*\{(.*?)\}\s*"
                     r"gg_plan_joinkind;", src, re.S).group(1)
    return {m.group(1): int(m.group(2))
            for m in re.finditer(r"(GG_JOIN_\w+)\s*=\s*(\d+)", body)}


def test_joinkind_constants_match_header():
    import greengage_amd
    from greengage_amd import engine as ge
    vals = _enum_values()
    assert vals == {"GG_JOIN_SEMI": 0, "GG_JOIN_INNER": 1}
    assert ge.JOIN_SEMI == vals["GG_JOIN_SEMI"]
    assert ge.JOIN_INNER == vals["GG_JOIN_INNER"]
    assert (greengage_amd.JOIN_SEMI, greengage_amd.JOIN_INNER) == (0, 1)


def test_plan_desc_layout_matches_library():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()


def test_new_fields_default_to_todays_meaning():
    """a zero-initialised descriptor says SEMI joins and driving-table
    sources everywhere"""
    from greengage_amd import engine as ge
    d = ge._PlanDesc()
    assert [j.kind for j in d.joins] == [ge.JOIN_SEMI] * 2
    assert [j.probe_src for j in d.joins] == [0, 0]
    assert list(d.group_src) == [0, 0]
    assert all(list(a.src) == [0, 0, 0] for a in d.aggs)
