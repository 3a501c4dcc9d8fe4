"""Per-aggregate FILTER predicates, the parts that need no GPU: the
binding's mirror of gg_plan_filter against include/engine_abi.h and the
built library, the descriptor builder's filter de-duplication, the
reference evaluator against a brute-force loop, and the properties the
fuzz seed (plan_filter_gen.SEED) was chosen for."""
import ctypes
import os
import re

import numpy as np
import pytest

import plan_filter_gen as gen
from plan_filter_ref import NEG_INF, NULL_KEY, POS_INF, eval_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        src = f.read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


def test_plan_desc_layout_matches_library():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()
    assert hasattr(ge._PlanDesc, "filters") and hasattr(ge._PlanDesc,
                                                         "nfilters")


def test_plan_agg_size_unchanged():
    """`filter` sits in what was tail padding after src[3]: two ints,
    three pointers, 3 + 3 bytes rounded up to the pointer alignment"""
    from greengage_amd import engine as ge
    ptr = ctypes.sizeof(ctypes.c_char_p)
    before = 2 * ctypes.sizeof(ctypes.c_int) + 3 * ptr + 6
    before += -before % ptr
    assert before == 40
    assert ctypes.sizeof(ge._PlanAgg) == before
    assert ge._PlanAgg.filter.offset == ge._PlanAgg.src.offset + 3


def test_filter_constants_match_header():
    import greengage_amd
    from greengage_amd import engine as ge
    assert ge.PLAN_MAX_FILTERS == _define("GG_PLAN_MAX_FILTERS") == 4
    assert ge.PLAN_MAX_FILTER_PREDS == _define("GG_PLAN_MAX_FILTER_PREDS") == 4
    assert greengage_amd.PLAN_MAX_FILTERS == ge.PLAN_MAX_FILTERS
    assert greengage_amd.PLAN_MAX_FILTER_PREDS == ge.PLAN_MAX_FILTER_PREDS
    assert len(ge._PlanDesc().filters) == ge.PLAN_MAX_FILTERS
    assert len(ge._PlanFilter().preds) == ge.PLAN_MAX_FILTER_PREDS


def test_zero_descriptor_has_no_filters():
    from greengage_amd import engine as ge
    d = ge._PlanDesc()
    assert d.nfilters == 0
    assert all(a.filter == 0 for a in d.aggs)
    assert all(f.npreds == 0 and list(f.src) == [0] * 4 for f in d.filters)


def test_builder_without_filters_leaves_the_tail_zero():
    from greengage_amd import engine as ge
    d, kinds = ge.build_plan_desc(3, preds=[("a", 0, 5)], group_cols=["g"],
                                  aggs=["count", ("sum", [("a", "id")])])
    assert kinds == [ge.AGG_COUNT_STAR, ge.AGG_SUM]
    assert d.nfilters == 0 and [a.filter for a in d.aggs] == [0] * 8


def test_builder_deduplicates_filters():
    from greengage_amd import engine as ge
    f0 = [("a", 0, 5), ((0, "b"), NEG_INF, 7)]
    f1 = [("a", 0, 5)]
    d, kinds = ge.build_plan_desc(
        3, joins=[{"table": 4, "build_key": "k", "probe_key": "fk",
                   "kind": "inner"}],
        aggs=[("filter", ("sum", [("a", "id")]), f0),
              "count",
              ("filter", "count", f1),
              ("filter", ("min", ("a", "sub100")), list(f0)),
              ("filter", ("avg", [("a", "id")]), f1)])
    # the inner kinds, so execute_plan decodes as ever
    assert kinds == [ge.AGG_SUM, ge.AGG_COUNT_STAR, ge.AGG_COUNT_STAR,
                     ge.AGG_MIN, ge.AGG_AVG]
    assert d.nfilters == 2
    assert [d.aggs[a].filter for a in range(5)] == [1, 0, 2, 1, 2]
    assert d.filters[0].npreds == 2 and d.filters[1].npreds == 1
    p = d.filters[0].preds
    assert (p[0].col, p[0].lo, p[0].hi) == (b"a", 0, 5)
    assert (p[1].col, p[1].lo, p[1].hi) == (b"b", NEG_INF, 7)
    assert list(d.filters[0].src)[:2] == [0, 1]
    assert list(d.filters[1].src)[:1] == [0]
    # same columns and bounds in another order are another conjunction
    # list: no attempt at normalising
    d2, _ = ge.build_plan_desc(3, aggs=[
        ("filter", "count", [("a", 0, 5), ("b", 1, 2)]),
        ("filter", "count", [("b", 1, 2), ("a", 0, 5)])])
    assert d2.nfilters == 2


def test_builder_refuses_a_fifth_distinct_filter():
    from greengage_amd import engine as ge
    aggs = [("filter", "count", [("a", v, v + 1)]) for v in range(5)]
    d, _ = ge.build_plan_desc(3, aggs=aggs[:4])
    assert d.nfilters == 4
    with pytest.raises(ValueError):
        ge.build_plan_desc(3, aggs=aggs)
    # four distinct lists, used eight times: fine
    d, _ = ge.build_plan_desc(3, aggs=aggs[:4] + aggs[:4])
    assert d.nfilters == 4
    assert [a.filter for a in d.aggs] == [1, 2, 3, 4, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        ge.build_plan_desc(3, aggs=[
            ("filter", "count", [("a", v, v + 1) for v in range(5)])])


# ---- the evaluator against a brute-force loop ----

def _tables():
    rng = np.random.default_rng(7)
    n, m = 40, 6
    data = {"g": rng.integers(0, 4, n), "x": rng.integers(-50, 50, n),
            "y": rng.integers(0, 10, n), "fk": rng.integers(0, 8, n)}
    nulls = {c: np.zeros(n, bool) for c in data}
    nulls["y"] = rng.random(n) < 0.25
    nulls["x"][::7] = True
    # group 3: every row fails the filter y in [0, 10) through NULLs
    nulls["y"][data["g"] == 3] = True
    # group 2: every row fails the payload filter (its partners have w = 9)
    data["fk"][data["g"] == 2] = 5
    bdata = {"k": np.arange(m), "w": np.array([1, 2, 3, 4, 5, 9]),
             "z": rng.integers(-5, 5, m)}
    bnulls = {c: np.zeros(m, bool) for c in bdata}
    bnulls["w"][1] = True
    return n, data, nulls, bdata, bnulls


def _brute(n, data, nulls, bdata, bnulls, wh, aggs):
    """INNER join on fk = k, WHERE x-range `wh`, group by g; aggs are
    (kind, column source, column, filter [(source, col, lo, hi)])"""
    groups = {}
    for i in range(n):
        if nulls["x"][i] or not wh[0] <= data["x"][i] < wh[1]:
            continue
        r = [b for b in range(len(bdata["k"])) if bdata["k"][b] == data["fk"][i]]
        if not r:
            continue
        view = {0: (data, nulls, i), 1: (bdata, bnulls, r[0])}
        acc = groups.setdefault(int(data["g"][i]), [[] for _ in aggs])
        for a, (kind, src, col, flt) in enumerate(aggs):
            ok = all(not view[s][1][c][view[s][2]] and
                     lo <= view[s][0][c][view[s][2]] < hi
                     for s, c, lo, hi in flt)
            if not ok:
                continue
            if kind == "count*":
                acc[a].append(1)
            elif not view[src][1][col][view[src][2]]:
                acc[a].append(int(view[src][0][col][view[src][2]]))
    out = []
    for g in sorted(groups):
        vals = []
        for (kind, *_), v in zip(aggs, groups[g]):
            vals.append(len(v) if kind in ("count*", "count")
                        else sum(v) if kind == "sum"
                        else (sum(v), len(v)) if kind == "avg"
                        else None if not v
                        else min(v) if kind == "min" else max(v))
        out.append((g, 0, vals))
    return out


def test_evaluator_matches_brute_force():
    n, data, nulls, bdata, bnulls = _tables()
    f_y = [(0, "y", 0, 10)]                  # fails on every NULL y
    f_w = [(1, "w", NEG_INF, 6)]             # payload, one NULL flag
    f_mix = [(0, "y", 2, POS_INF), (1, "z", -3, 3)]
    brute_aggs = [("count*", 0, None, []), ("count*", 0, None, f_y),
                  ("sum", 0, "x", f_y), ("min", 0, "x", f_y),
                  ("avg", 1, "z", f_w), ("count", 0, "y", f_w),
                  ("max", 1, "w", f_mix), ("sum", 0, "x", [])]

    def col(s, c):
        return c if s == 0 else (0, c)

    def flt(f):
        return [(col(s, c), lo, hi) for s, c, lo, hi in f]

    aggs = ["count", ("filter", "count", flt(f_y)),
            ("filter", ("sum", [("x", "id")]), flt(f_y)),
            ("filter", ("min", ("x", "id")), flt(f_y)),
            ("filter", ("avg", [((0, "z"), "id")]), flt(f_w)),
            ("filter", ("count", "y"), flt(f_w)),
            ("filter", ("max", ((0, "w"), "id")), flt(f_mix)),
            ("sum", [("x", "id")])]
    joins = [{"build_key": "k", "probe_key": "fk", "kind": "inner",
              "_data": bdata, "_nulls": bnulls, "_n": len(bdata["k"])}]
    wh = (-40, 45)
    got = eval_plan(n, data, nulls, [("x",) + wh], joins, ["g"], aggs)
    exp = _brute(n, data, nulls, bdata, bnulls, wh, brute_aggs)
    assert got == exp
    by = {g: v for g, _k1, v in got}
    # the groups built to fail a filter are present and report the
    # contract's empty values beside live unfiltered twins
    assert by[3][0] > 0 and by[3][1:4] == [0, 0, None]
    assert by[2][0] > 0 and by[2][4] == (0, 0) and by[2][5] == 0
    # a plain aggregate yields one row even when nothing passes
    one = eval_plan(n, data, nulls, [("x", 1000, 1001)], joins, [],
                    aggs[:4])
    assert one == [(0, 0, [0, 0, 0, None])]
    # NULL group keys group together, filters notwithstanding
    nulls["g"][:3] = True
    got = eval_plan(n, data, nulls, [], joins, ["g"], aggs[:2])
    assert got[0][0] == NULL_KEY


# ---- what the fuzz seed was chosen for ----

def test_fuzz_seed_properties():
    descs = gen.all_descs()
    assert len(descs) == gen.NDESC == 16
    for d in descs:
        assert 0 <= len(d["joins"]) <= 2 and 0 <= len(d["group"]) <= 2
        assert 1 <= len(d["aggs"]) <= 4
        assert gen.slots(d) <= gen.MAX_SLOTS, d["it"]
    assert sum(gen.references_filter(d) for d in descs) >= 10
    assert sum(gen.filters_on_payload(d) for d in descs) >= 4
    assert sum(gen.has_empty_pair(d) for d in descs) >= 3
    kinds = set()
    for d in descs:
        for a in d["aggs"]:
            a = a[1] if a[0] == "filter" else a
            kinds.add(a if a == "count" else
                      "count_col" if a[0] == "count" else a[0])
    assert kinds == {"count", "count_col", "sum", "min", "max", "avg"}
