"""General WHERE clauses of compiled plans (engine_abi.h gg_plan_where),
without a GPU: the extension's layout in the binding's mirror, the untouched
descriptor, the builder's sugar and limits, the reference (plan_where_ref)
against hand-written expectations and against its naive Kleene evaluator,
and what plan_where_gen's seed was chosen for.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import plan_where_gen as gen
from plan_where_ref import (eval_plan, k_and, k_not, k_or, naive_plan,
                            row_masks)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _header():
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        return f.read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, _header()).group(1))


def _plain(v):
    """a ctypes value as plain Python data (strings by value)"""
    if isinstance(v, ctypes.Structure):
        return {f: _plain(getattr(v, f)) for f, _t in v._fields_}
    if isinstance(v, ctypes.Array):
        return [_plain(x) for x in v]
    return v


def _atoms(w):
    """the used part of a _PlanWhere: [(scope, [(kind, col, src, col2, src2,
    lo, hi)])]"""
    return [(w.clauses[c].scope,
             [(a.kind, a.col, a.src, a.col2, a.src2, a.lo, a.hi)
              for a in list(w.clauses[c].atoms)[:w.clauses[c].natoms]])
            for c in range(w.nclauses)]


# ---- layout ----

def test_where_layout_matches_library():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanWhere) == ge.lib().gg_engine_plan_where_size()
    assert [f for f, _t in ge._PlanAtom._fields_] == [
        "col", "col2", "lo", "hi", "kind", "src", "src2"]
    assert [f for f, _t in ge._PlanClause._fields_] == [
        "atoms", "natoms", "scope"]
    assert [f for f, _t in ge._PlanWhere._fields_] == ["clauses", "nclauses"]
    assert ctypes.sizeof(ge._PlanAtom) == 40
    assert ge._PlanClause.natoms.offset == 40 * ge.PLAN_MAX_ATOMS
    assert ge._PlanClause.scope.offset == 40 * ge.PLAN_MAX_ATOMS + 4


def test_constants_match_header():
    import greengage_amd as g
    from greengage_amd import engine as ge
    assert ge.PLAN_MAX_CLAUSES == _define("GG_PLAN_MAX_CLAUSES") == 8
    assert ge.PLAN_MAX_ATOMS == _define("GG_PLAN_MAX_ATOMS") == 8
    assert ge.PLAN_MAX_WHERE_ATOMS == _define("GG_PLAN_MAX_WHERE_ATOMS") == 16
    assert g.PLAN_MAX_CLAUSES == 8 and g.PLAN_MAX_WHERE_ATOMS == 16
    src = _header()
    for name in ("RANGE", "NOT_RANGE", "LT", "LE", "EQ", "NE", "IS_NULL",
                 "NOT_NULL"):
        v = int(re.search(r"GG_ATOM_%s\s*=\s*(\d+)" % name, src).group(1))
        assert getattr(ge, "ATOM_" + name) == v == getattr(g, "ATOM_" + name)


def test_plan_desc_is_untouched():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()
    assert [f for f, _t in ge._PlanDesc._fields_][-1] == "est_groups"
    join = {"table": 4, "build_key": "k", "probe_key": "a", "kind": "left",
            "preds": [("k", 0, 9)]}
    args = dict(preds=[("a", 0, 5)], group_cols=["g", (0, "h")],
                aggs=["count", ("filter", ("sum", [("a", "id")]),
                                [("a", 1, 3)])],
                order_by=[("agg", 0, "desc")], limit=3, est_groups=7)
    d0, k0 = ge.build_plan_desc(7, joins=[join], **args)
    d1, k1 = ge.build_plan_desc(
        7, joins=[dict(join, where=[("is_null", "k")])], **args)
    assert k0 == k1 and _plain(d0) == _plain(d1)


# ---- the builder ----

def test_builder_sugar():
    from greengage_amd import engine as ge
    w = ge.build_plan_where(
        [{"where": [("eq", "bk", 3)]}, {}],
        [("range", "a", 1, 5),
         [("not_range", (0, "x"), 2, 4), ("is_null", (1, "y")),
          ("not_null", "a")],
         ("ne", "a", 7),
         [("in", "a", [4, 6, 9]), ("eq", "b", -1)],
         ("not_in", "c", [1, 2]),
         ("cmp", "a", "<>", (0, "x"))])
    R, NR = ge.ATOM_RANGE, ge.ATOM_NOT_RANGE
    assert _atoms(w) == [
        (0, [(R, b"a", 0, None, 0, 1, 5)]),
        (0, [(NR, b"x", 1, None, 0, 2, 4),
             (ge.ATOM_IS_NULL, b"y", 2, None, 0, 0, 0),
             (ge.ATOM_NOT_NULL, b"a", 0, None, 0, 0, 0)]),
        (0, [(NR, b"a", 0, None, 0, 7, 8)]),
        (0, [(R, b"a", 0, None, 0, 4, 5), (R, b"a", 0, None, 0, 6, 7),
             (R, b"a", 0, None, 0, 9, 10), (R, b"b", 0, None, 0, -1, 0)]),
        (0, [(NR, b"c", 0, None, 0, 1, 2)]),
        (0, [(NR, b"c", 0, None, 0, 2, 3)]),
        (0, [(ge.ATOM_NE, b"a", 0, b"x", 1, 0, 0)]),
        (1, [(R, b"bk", 0, None, 0, 3, 4)])]


def test_builder_compare_ops_and_swap():
    from greengage_amd import engine as ge
    got = {}
    for op in ("<", "<=", "=", "<>", ">", ">="):
        w = ge.build_plan_where((), [("cmp", "a", op, (1, "b"))])
        (_s, [(kind, col, src, col2, src2, _lo, _hi)]), = _atoms(w)
        got[op] = (kind, col, src, col2, src2)
    assert got == {"<": (ge.ATOM_LT, b"a", 0, b"b", 2),
                   "<=": (ge.ATOM_LE, b"a", 0, b"b", 2),
                   "=": (ge.ATOM_EQ, b"a", 0, b"b", 2),
                   "<>": (ge.ATOM_NE, b"a", 0, b"b", 2),
                   ">": (ge.ATOM_LT, b"b", 2, b"a", 0),
                   ">=": (ge.ATOM_LE, b"b", 2, b"a", 0)}


def test_builder_limits_raise():
    from greengage_amd import engine as ge
    one = ("eq", "a", 1)
    assert ge.build_plan_where((), [one] * 8).nclauses == 8
    with pytest.raises(ValueError):
        ge.build_plan_where((), [one] * 9)
    with pytest.raises(ValueError):        # a join's clauses count too
        ge.build_plan_where([{"where": [one] * 5}], [one] * 4)
    assert ge.build_plan_where((), [[one] * 8]).clauses[0].natoms == 8
    with pytest.raises(ValueError):
        ge.build_plan_where((), [[one] * 9])
    with pytest.raises(ValueError):        # an IN-list counts per value
        ge.build_plan_where((), [("in", "a", list(range(9)))])
    assert ge.build_plan_where((), [[one] * 8, [one] * 8]).nclauses == 2
    with pytest.raises(ValueError):        # 17 atoms in all
        ge.build_plan_where((), [[one] * 8, [one] * 8, one])
    with pytest.raises(ValueError):
        ge.build_plan_where((), [("not_in", "a", list(range(9)))])


def test_no_clause_is_no_extension():
    from greengage_amd import engine as ge
    assert ge.build_plan_where().nclauses == 0
    assert ge.build_plan_where([{"table": 1}, {"where": []}], ()).nclauses == 0
    assert _plain(ge.build_plan_where()) == _plain(ge._PlanWhere())


# ---- the reference against hand-written expectations ----

#          row:   0     1     2     3     4     5
A = np.array([3, 7, 5, 0, 9, 5], np.int64)
AN = np.array([0, 0, 0, 1, 0, 1], bool)
B = np.array([5, 5, 5, 5, 0, 0], np.int64)
BN = np.array([0, 0, 1, 0, 0, 1], bool)     # NULL on b: row 2; on both: row 5
DATA = {"a": A, "b": B}
NULLS = {"a": AN, "b": BN}


def _kept(where, evaluator=eval_plan):
    """rows a COUNT(*) grouped by nothing sees, as the surviving row set"""
    _m0, m, _r = row_masks(6, DATA, NULLS, [], [], where)
    n = evaluator(6, DATA, NULLS, [], [], [], ["count"], where)[0][2][0]
    assert n == int(m.sum())
    return sorted(np.nonzero(m)[0].tolist())


@pytest.mark.parametrize("evaluator", [eval_plan, naive_plan])
def test_every_atom_kind_by_hand(evaluator):
    k = lambda w: _kept(w, evaluator)           # noqa: E731
    assert k([("range", "a", 3, 7)]) == [0, 2]
    assert k([("not_range", "a", 3, 7)]) == [1, 4]
    assert k([("eq", "a", 5)]) == [2]
    assert k([("ne", "a", 5)]) == [0, 1, 4]
    assert k([("in", "a", [3, 9, 0])]) == [0, 4]
    assert k([("not_in", "a", [3, 9])]) == [1, 2]
    assert k([("cmp", "a", "<", "b")]) == [0]
    assert k([("cmp", "a", "<=", "b")]) == [0]
    assert k([("cmp", "a", "=", "b")]) == []
    assert k([("cmp", "a", "<>", "b")]) == [0, 1, 4]
    assert k([("cmp", "a", ">", "b")]) == [1, 4]
    assert k([("cmp", "a", ">=", "b")]) == [1, 4]
    assert k([("is_null", "a")]) == [3, 5]
    assert k([("not_null", "a")]) == [0, 1, 2, 4]
    assert k([("is_null", "b")]) == [2, 5]
    # a IS NULL OR a < 5
    assert k([[("is_null", "a"), ("range", "a", INT64_MIN, 5)]]) == [0, 3, 5]
    # (a < b OR b IS NULL) AND a IS NOT NULL
    assert k([[("cmp", "a", "<", "b"), ("is_null", "b")],
              ("not_null", "a")]) == [0, 2]
    # literal bounds: NOT_RANGE is the complement on non-NULL values
    assert k([("not_range", "a", INT64_MIN, INT64_MAX)]) == []
    assert k([("range", "a", INT64_MIN, INT64_MAX)]) == [0, 1, 2, 4]


def test_kleene_tables():
    T, F, N = True, False, None
    assert [k_not(x) for x in (T, F, N)] == [F, T, N]
    assert k_or([F, N]) is N and k_or([N, T]) is T and k_or([F, F]) is F
    assert k_and([T, N]) is N and k_and([N, F]) is F and k_and([T, T]) is T
    assert k_or([]) is F and k_and([]) is T


def test_where_decides_groups_filter_does_not():
    g = {"a": A, "b": B, "g": np.array([0, 0, 1, 1, 2, 2], np.int64)}
    gn = dict(NULLS, g=np.zeros(6, bool))
    flt = [("filter", "count", [("a", 0, 6)])]
    assert eval_plan(6, g, gn, [], [], ["g"], flt) == [
        (0, 0, [1]), (1, 0, [1]), (2, 0, [0])]
    for ev in (eval_plan, naive_plan):
        assert ev(6, g, gn, [], [], ["g"], ["count"],
                  [("range", "a", 0, 6)]) == [(0, 0, [1]), (1, 0, [1])]
        assert ev(6, g, gn, [], [], [], ["count"],
                  [("range", "a", 100, 101)]) == [(0, 0, [0])]


# ---- the fuzz descriptors ----

@pytest.fixture(scope="module")
def descs():
    return gen.all_descs()


def test_vectorised_reference_equals_naive_kleene(descs):
    assert len(descs) == gen.NDESC == 16
    for d in descs:
        assert gen.expected(d) == gen.expected(d, evaluator=naive_plan), \
            d["it"]


def test_seed_properties(descs):
    p = gen.properties(descs)
    assert p["kinds"] == set(range(8)), p
    assert p["scan"] >= 4 and p["post"] >= 4 and p["build"] >= 4, p
    assert p["left_null"] >= 3, p
    assert p["mixed"] >= 3, p
    assert p["drops_and_keeps"] >= 12, p
    assert p["empty"] == 0, p
    assert gen.properties_hold(p)
