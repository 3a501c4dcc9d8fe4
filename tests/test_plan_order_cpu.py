"""ORDER BY / LIMIT / est_groups of compiled plans, without a GPU: the
descriptor's new tail in the binding's mirror, the zero tail of default
arguments, the binding's NULL-placement defaults, and the reference sorter
(plan_order_ref) against hand-written expectations.
"""
import ctypes
import os
import re

import pytest

from plan_order_ref import NULL_KEY, order_groups

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        src = f.read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


# ---- layout ----

def test_plan_desc_layout_matches_library():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()


def test_tail_follows_nfilters_in_header_order():
    from greengage_amd import engine as ge
    D = ge._PlanDesc
    assert ctypes.sizeof(ge._PlanOrder) == 4
    assert [f for f, _t in ge._PlanOrder._fields_] == [
        "what", "index", "desc", "nulls_first"]
    # int nfilters; 4 x 4-byte entries; int norder; two aligned int64
    assert D.order.offset == D.nfilters.offset + 4
    assert D.norder.offset == D.order.offset + 4 * ge.PLAN_MAX_ORDER
    assert D.limit.offset == (D.norder.offset + 4 + 7) // 8 * 8
    assert D.est_groups.offset == D.limit.offset + 8
    assert ctypes.sizeof(D) == D.est_groups.offset + 8
    names = [f for f, _t in D._fields_]
    assert names[-5:] == ["nfilters", "order", "norder", "limit",
                          "est_groups"]


def test_constants_match_header():
    import greengage_amd
    from greengage_amd import engine as ge
    assert ge.PLAN_MAX_ORDER == _define("GG_PLAN_MAX_ORDER") == 4
    assert ge.PLAN_MAX_LIMIT == _define("GG_PLAN_MAX_LIMIT") == 1024
    assert greengage_amd.PLAN_MAX_LIMIT == ge.PLAN_MAX_LIMIT
    assert len(ge._PlanDesc().order) == ge.PLAN_MAX_ORDER


def test_topk_tile_is_exported_and_holds_two_limits():
    from greengage_amd import engine as ge
    t = ge.plan_topk_tile()
    assert t >= 2 * ge.PLAN_MAX_LIMIT and t & (t - 1) == 0


# ---- the builder ----

ARGS = dict(preds=[("a", 0, 5)], group_cols=["g", (0, "h")],
            joins=[{"table": 4, "build_key": "k", "probe_key": "a",
                    "kind": "left"}],
            aggs=["count", ("filter", ("sum", [("a", "id")]),
                            [("a", 1, 3)]), ("min", ("a", "id"))])


def _plain(v):
    """a ctypes value as plain Python data (strings by value: every call of
    the builder holds its own copies, so the raw pointers differ)"""
    if isinstance(v, ctypes.Structure):
        return {f: _plain(getattr(v, f)) for f, _t in v._fields_}
    if isinstance(v, ctypes.Array):
        return [_plain(x) for x in v]
    return v


def test_default_arguments_leave_the_tail_zero():
    """... byte for byte, and the fields before it are what the builder
    produced before it knew of an order: spelling the defaults out, or
    adding an order, changes none of them"""
    from greengage_amd import engine as ge
    old = [f for f, _t in ge._PlanDesc._fields_][:-4]
    assert old[-1] == "nfilters"
    d, kinds = ge.build_plan_desc(3, **ARGS)
    tail = ge._PlanDesc.order.offset
    raw = bytes(d)
    assert raw[tail:] == bytes(len(raw) - tail)
    assert d.norder == 0 and d.limit == 0 and d.est_groups == 0
    e, kinds_e = ge.build_plan_desc(3, order_by=(), limit=0, est_groups=0,
                                    **ARGS)
    assert bytes(e)[tail:] == raw[tail:] and kinds == kinds_e
    o, kinds_o = ge.build_plan_desc(3, order_by=[("agg", 0, "desc")],
                                    limit=7, est_groups=9, **ARGS)
    assert (o.norder, o.limit, o.est_groups) == (1, 7, 9)
    assert kinds_o == kinds
    pd, pe, po = _plain(d), _plain(e), _plain(o)
    for f in old:
        assert pd[f] == pe[f] == po[f], f
    # and the prefix holds what was asked for
    assert pd["group_cols"] == [b"g", b"h"] and pd["group_src"] == [0, 1]
    assert pd["aggs"][1]["filter"] == 1 and pd["nfilters"] == 1
    assert pd["joins"][0]["kind"] == ge.JOIN_LEFT


def test_null_placement_defaults_are_postgres():
    from greengage_amd import engine as ge
    d, _ = ge.build_plan_desc(
        3, group_cols=["g"], aggs=["count", ("max", ("a", "id"))],
        order_by=[("agg", 1, "asc"), ("agg", 1, "desc"),
                  ("key", 0, "asc", "nulls_first"),
                  ("key", 0, "desc", "nulls_last")])
    got = [(o.what, o.index, o.desc, o.nulls_first) for o in d.order]
    assert got == [(1, 1, 0, 0),      # ASC: NULLS LAST
                   (1, 1, 1, 1),      # DESC: NULLS FIRST
                   (0, 0, 0, 1), (0, 0, 1, 0)]
    assert d.norder == 4


def test_builder_refuses_a_fifth_order_entry():
    from greengage_amd import engine as ge
    with pytest.raises(ValueError):
        ge.build_plan_desc(3, aggs=["count"],
                           order_by=[("agg", 0, "asc")] * 5)


# ---- the reference sorter, against expectations written by hand ----

N = NULL_KEY
#          key0 key1  [COUNT, SUM, MAX]
G = [(1, 0, [2, 10, 5]),
     (2, 0, [2, -3, None]),
     (3, 0, [1, 1 << 70, 7]),
     (N, 0, [2, 10, None]),
     (5, 0, [1, -(1 << 70), 7])]


def _k(groups):
    return [g[0] for g in groups]


def test_sorter_default_is_key_order_null_key_first():
    assert _k(order_groups(G)) == [N, 1, 2, 3, 5]
    assert _k(order_groups(G, limit=2)) == [N, 1]
    assert _k(order_groups(G, limit=99)) == [N, 1, 2, 3, 5]


def test_sorter_ties_fall_back_to_keys_ascending_even_under_desc():
    # COUNT ties: 2 -> {N, 1, 2}, 1 -> {3, 5}
    assert _k(order_groups(G, [("agg", 0, "asc")])) == [3, 5, N, 1, 2]
    assert _k(order_groups(G, [("agg", 0, "desc")])) == [N, 1, 2, 3, 5]


def test_sorter_sums_compare_as_big_ints():
    assert _k(order_groups(G, [("agg", 1, "asc")])) == [5, 2, N, 1, 3]
    assert _k(order_groups(G, [("agg", 1, "desc")], limit=3)) == [3, N, 1]


def test_sorter_null_max_follows_placement_not_direction():
    # MAX: 5 -> 1; 7 -> {3, 5}; NULL -> {N, 2}
    assert _k(order_groups(G, [("agg", 2, "asc")])) == [1, 3, 5, N, 2]
    assert _k(order_groups(G, [("agg", 2, "asc", "nulls_first")])) == [
        N, 2, 1, 3, 5]
    assert _k(order_groups(G, [("agg", 2, "desc")])) == [N, 2, 3, 5, 1]
    assert _k(order_groups(G, [("agg", 2, "desc", "nulls_last")])) == [
        3, 5, 1, N, 2]


def test_sorter_null_key_follows_placement_not_direction():
    assert _k(order_groups(G, [("key", 0, "asc")])) == [1, 2, 3, 5, N]
    assert _k(order_groups(G, [("key", 0, "asc", "nulls_first")])) == [
        N, 1, 2, 3, 5]
    assert _k(order_groups(G, [("key", 0, "desc")])) == [N, 5, 3, 2, 1]
    assert _k(order_groups(G, [("key", 0, "desc", "nulls_last")])) == [
        5, 3, 2, 1, N]


def test_sorter_later_entries_decide_among_ties():
    by = [("agg", 0, "desc"), ("agg", 2, "asc", "nulls_first"),
          ("agg", 1, "asc")]
    # COUNT 2: MAX NULL {2 (SUM -3), N (SUM 10)}, then 1; COUNT 1: MAX 7
    # {5 (SUM -2^70), 3 (SUM 2^70)}
    assert _k(order_groups(G, by)) == [2, N, 1, 5, 3]
    assert _k(order_groups(G, by, limit=1)) == [2]


def test_sorter_second_key_breaks_ties():
    g = [(1, 9, [0]), (1, N, [0]), (1, -4, [0]), (0, 5, [0])]
    assert [(a, b) for a, b, _v in order_groups(g, [("agg", 0, "desc")])] \
        == [(0, 5), (1, N), (1, -4), (1, 9)]
    assert [(a, b) for a, b, _v in order_groups(g, [("key", 1, "desc")])] \
        == [(1, N), (1, 9), (0, 5), (1, -4)]
