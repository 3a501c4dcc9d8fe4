"""General WHERE clauses of compiled plans (engine_abi.h gg_plan_where),
directed cases: OR / IN / NOT, column-against-column comparisons, also
across a join, IS [NOT] NULL, and the build-scope clauses of every join kind.

Every case runs on the generated kernels and, under plan_mode("interp"), on
the interpreted kernel, three executes each unless noted (the baked kernel
takes over from the second where one is made), and must equal
plan_where_ref.eval_plan bit for bit.

Shapes are the smallest at which the kernels can still go wrong: driving
rows 0, 1 and 257 (nothing; one thread; a second block holding one row),
one table of 4 * 2048 * 256 + 777 rows (the smallest at which the
interpreted kernel's 4-way strided loop runs as well as its tail), build
tables of 0, 3 and 300 rows.
"""
import ctypes

import numpy as np
import pytest

from plan_order_ref import order_groups
from plan_where_ref import (NEG_INF, eval_plan, join, plan_mode, register,
                            run, strip)

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = 1, 5
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OPS = ["<", "<=", "=", "<>", ">", ">="]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


@pytest.fixture(params=["rtc", "interp"])
def mode(request):
    return request.param


def wjoin(*a, where=(), **kw):
    """plan_where_ref.join with build-scope clauses"""
    return dict(join(*a, **kw), where=list(where))


def _check_paths(paths, mode, where=True):
    assert ("path_plan_interp" if mode == "interp" else "path_plan_rtc") \
        in paths
    assert ("path_plan_where" in paths) == where


def _count(exp):
    return sum(v[0] for _a, _b, v in exp)


# ---- sizes ----

@pytest.mark.parametrize("n", [0, 1, 257])
def test_sizes(eng, mode, n):
    rng = np.random.default_rng(100 + n)
    t, d, nl = register(eng, f"pw_sz_{n}_{mode}", [
        ("a", "int32", rng.integers(0, 10, n).astype(np.int32)),
        ("b", "int64", rng.integers(0, 10, n).astype(np.int64)),
        ("g", "char1", rng.integers(0, 3, n).astype(np.uint8))],
        {"a": rng.random(n) < 0.2} if n else None)
    where = [[("cmp", "a", "<=", "b"), ("is_null", "a")], ("ne", "b", 3)]
    aggs = ["count", ("sum", [("b", "id")])]
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], [], aggs, where)
    _check_paths(paths, mode)
    assert len(exp) == 1
    if n:
        _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["g"], aggs, where)


def test_both_scan_loops(eng):
    """the strided loop and the tail, with a scan clause and a post-join
    clause.  Generated kernels, two executes; one interpreted execute."""
    rng = np.random.default_rng(21)
    m, n = 1_000, 4 * 2048 * 256 + 777
    keys = ((rng.permutation(np.arange(m)) - 100) * 5 + 2).astype(np.int32)
    bt, bd, bn = register(eng, "pw_big_b", [
        ("bk", "int32", keys),
        ("cat", "int32", rng.integers(0, 6, m).astype(np.int32)),
        ("lim", "int32", rng.integers(0, 900, m).astype(np.int32))],
        {"lim": rng.random(m) < 0.1})
    t, d, nl = register(eng, "pw_big_d", [
        ("fk", "int32", rng.integers(-600, 5 * m, n).astype(np.int32)),
        ("v", "int32", rng.integers(-9, 1000, n).astype(np.int32)),
        ("u", "char1", rng.integers(0, 256, n).astype(np.uint8))],
        {"v": rng.random(n) < 0.05})
    j = join(bt, bd, bn, "bk", "fk", kind="left")
    where = [[("in", "u", [3, 200, 77]), ("cmp", "u", ">", "v"),
              ("is_null", "v")],
             [("cmp", "v", "<", (0, "lim")), ("is_null", (0, "lim"))]]
    aggs = [("sum", [("v", "id")]), "count"]
    exp = eval_plan(n, d, nl, [], [j], [(0, "cat")], aggs, where)
    assert len(exp) == 7 and 0 < _count([(a, b, v[1:]) for a, b, v in exp]) < n
    run(eng, "rtc", t, d, nl, [], [j], [(0, "cat")], aggs, where, repeats=2,
        exp=exp)
    run(eng, "interp", t, d, nl, [], [j], [(0, "cat")], aggs, where,
        repeats=1, exp=exp)


# ---- constants, compares, NULLs ----

WIDTHS = [("char1", np.uint8, 0, 256), ("int32", np.int32, -40, 40),
          ("int64", np.int64, -40, 40)]


@pytest.fixture(scope="module")
def wide(eng):
    """per width a nullable column n<w> and a plain one p<w>; 257 rows, so
    NULL on a, on b and on both all occur"""
    rng = np.random.default_rng(7)
    n = 257
    cols, nullmap = [], {}
    for w, (ty, dt, lo, hi) in enumerate(WIDTHS):
        cols.append((f"n{w}", ty, rng.integers(lo, hi, n).astype(dt)))
        cols.append((f"p{w}", ty, rng.integers(lo, hi, n).astype(dt)))
        cols.append((f"m{w}", ty, rng.integers(lo, hi, n).astype(dt)))
        nullmap[f"n{w}"] = rng.random(n) < 0.3
        nullmap[f"m{w}"] = rng.random(n) < 0.3
    return register(eng, "pw_wide", cols, nullmap)


@pytest.mark.parametrize("w", range(3))
def test_every_kind_over_each_width(eng, mode, wide, w):
    t, d, nl = wide
    a = f"n{w}"
    lo, hi = (100, 180) if w == 0 else (-10, 15)
    cases = [[("range", a, lo, hi)], [("not_range", a, lo, hi)],
             [("is_null", a)], [("not_null", a)],
             [("is_null", f"p{w}")], [("not_null", f"p{w}")],
             # flag on a, on b, on both; b of every width
             [("cmp", a, "<", "m0")], [("cmp", a, "<=", "m1")],
             [("cmp", a, "=", "m2")], [("cmp", a, "<>", f"m{w}")],
             [("cmp", a, ">", f"p{(w + 1) % 3}")],
             [[("is_null", a), ("range", a, NEG_INF, 5)]]]
    for where in cases:
        _p, _exp, paths = run(eng, mode, t, d, nl, [], [], [],
                              ["count", ("count", a)], where)
        _check_paths(paths, mode)


def test_char1_above_127_against_negative_int32(eng, mode):
    c = np.array([0, 127, 128, 200, 255, 255, 1, 130], np.uint8)
    i = np.array([-1, -128, -128, -56, -1, 255, 1, 131], np.int32)
    t, d, nl = register(eng, f"pw_c1_{mode}", [("c", "char1", c),
                                               ("i", "int32", i)])
    got = {}
    for op in OPS:
        _p, exp, _paths = run(eng, mode, t, d, nl, [], [], [], ["count"],
                              [("cmp", "c", op, "i")])
        got[op] = exp[0][2][0]
    # char1 reads as 0..255: only rows 5 (=), 6 (=) and 7 (<) are not c > i
    assert got == {"<": 1, "<=": 3, "=": 2, "<>": 6, ">": 5, ">=": 7}


def test_int64_extremes(eng, mode):
    a = np.array([INT64_MIN, INT64_MAX, INT64_MIN, INT64_MAX, 0, -1],
                 np.int64)
    b = np.array([INT64_MAX, INT64_MIN, INT64_MIN, INT64_MAX, -1, 0],
                 np.int64)
    t, d, nl = register(eng, f"pw_ext_{mode}", [("a", "int64", a),
                                                ("b", "int64", b)])
    got = {}
    for op in OPS:              # > and >= are the swapped order
        _p, exp, _paths = run(eng, mode, t, d, nl, [], [], [], ["count"],
                              [("cmp", "a", op, "b")])
        got[op] = exp[0][2][0]
    assert got == {"<": 2, "<=": 4, "=": 2, "<>": 4, ">": 2, ">=": 4}
    for lo, hi, want in ((INT64_MIN, 0, 3), (0, INT64_MAX, 5),
                         (INT64_MIN, INT64_MAX, 2)):
        _p, exp, _paths = run(eng, mode, t, d, nl, [], [], [], ["count"],
                              [("not_range", "a", lo, hi)])
        assert exp[0][2][0] == want, (lo, hi)


# ---- limits ----

def test_limits(eng, mode, wide):
    t, d, nl = wide
    eight = [("in", "n1", list(range(-8, 8, 2)))]
    p, exp, _paths = run(eng, mode, t, d, nl, [], [], [], ["count"], eight)
    assert 0 < exp[0][2][0] < 257
    # the 8-value IN-list reads its int32 column once: 4 bytes per row
    scan = [s for s in eng.stats(p) if s["name"] == "plan_scan_agg"][0]
    assert scan["hbm_bytes_algorithmic"] == scan["launches"] * 257 * 4
    clauses = [("ne", "p1", v) for v in range(8)]
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["p0"], ["count"],
                          clauses)
    assert 0 < _count(exp) < 257
    sixteen = [[("in", "n1", list(range(0, 8)))],
               [("eq", "p2", v) for v in range(-4, 3)] + [("is_null", "n2")]]
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], [], ["count"], sixteen)
    assert exp[0][2][0] > 0


# ---- groups ----

def test_where_removes_a_group_filter_keeps_it(eng, mode):
    g = np.array([0, 0, 1, 1, 2, 2, 2], np.uint8)
    a = np.array([1, 9, 2, 3, 9, 9, 9], np.int32)
    t, d, nl = register(eng, f"pw_grp_{mode}", [("g", "char1", g),
                                                ("a", "int32", a)])
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["g"], ["count"],
                          [("range", "a", 0, 5)])
    assert exp == [(0, 0, [1]), (1, 0, [2])]
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["g"],
                         [("filter", "count", [("a", 0, 5)])])
    assert exp == [(0, 0, [1]), (1, 0, [2]), (2, 0, [0])]
    assert "path_plan_where" not in paths
    # ngroup == 0 with every row dropped: still one row
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], [],
                          ["count", ("min", ("a", "id"))],
                          [("eq", "a", 100)])
    assert exp == [(0, 0, [0, None])]


# ---- LEFT ----

def _left_tables(eng, tag, rng, n, m, style, present):
    keys = (np.arange(m) + 1 if style == "dense"
            else (np.arange(m) - m) * 1000 + 7).astype(np.int64)
    bt, bd, bn = register(eng, f"pw_lb_{tag}", [
        ("bk", "int64", keys),
        ("x", "int32", rng.integers(0, 100, m).astype(np.int32)),
        ("c", "char1", rng.integers(0, 3, m).astype(np.uint8))],
        {"x": rng.random(m) < 0.2} if m else None)
    absent = np.array([-5, 0, 1 << 40, int(keys.max()) + 3 if m else 9],
                      np.int64)
    pool = {"none": absent, "half": np.concatenate([keys, absent]),
            }[present]
    fk = rng.choice(pool, n)
    t, d, nl = register(eng, f"pw_ld_{tag}", [
        ("fk", "int64", fk),
        ("y", "int32", rng.integers(0, 100, n).astype(np.int32))],
        {"fk": rng.random(n) < 0.1})
    return t, d, nl, [join(bt, bd, bn, "bk", "fk", kind="left")]


@pytest.mark.parametrize("style", ["dense", "sparse"])
def test_left_all_null_extended(eng, mode, style):
    rng = np.random.default_rng(31)
    t, d, nl, joins = _left_tables(eng, f"all_{style}_{mode}", rng, 257, 300,
                                   style, "none")
    for where, want in (([("is_null", (0, "x"))], 257),
                        ([("not_null", (0, "x"))], 0),
                        ([("is_null", (0, "bk"))], 257),
                        ([("cmp", (0, "x"), "<>", "y")], 0)):
        _p, exp, paths = run(eng, mode, t, d, nl, [], joins, [],
                             ["count", ("count", (0, "x"))], where)
        assert exp[0][2][0] == want
        assert ("path_plan_join_index_dense" if style == "dense"
                else "path_plan_join_index_hash") in paths


@pytest.mark.parametrize("style", ["dense", "sparse"])
def test_left_half_extended(eng, mode, style):
    rng = np.random.default_rng(32)
    t, d, nl, joins = _left_tables(eng, f"half_{style}_{mode}", rng, 257,
                                   300, style, "half")
    where = [[("is_null", (0, "x")), ("range", (0, "x"), NEG_INF, 40)]]
    aggs = ["count", ("count", (0, "x")), ("sum", [((0, "x"), "id")])]
    _p, exp, paths = run(eng, mode, t, d, nl, [], joins, [(0, "c")], aggs,
                         where)
    _check_paths(paths, mode)
    # NULL-extended rows, flagged NULLs and small values all survive
    assert 0 < _count(exp) < 257 and any(v[0] > v[1] for _a, _b, v in exp)
    assert any(v[1] > 0 for _a, _b, v in exp)


def test_left_empty_build_table(eng, mode):
    rng = np.random.default_rng(33)
    t, d, nl, joins = _left_tables(eng, f"empty_{mode}", rng, 257, 0,
                                   "sparse", "none")
    _p, exp, _paths = run(eng, mode, t, d, nl, [], joins, [], ["count"],
                          [[("is_null", (0, "x")), ("eq", "y", 1)]])
    assert exp[0][2][0] == 257
    _p, exp, _paths = run(eng, mode, t, d, nl, [], joins, [], ["count"],
                          [("not_null", (0, "c"))])
    assert exp[0][2][0] == 0


# ---- cross-source ----

def test_cross_source_compares(eng, mode):
    rng = np.random.default_rng(41)
    n, m0, m1 = 257, 60, 40
    k1 = (np.arange(m1) * 7 - 50).astype(np.int32)          # hashed
    b1, b1d, b1n = register(eng, f"pw_x1_{mode}", [
        ("bk", "int32", k1),
        ("z", "int64", rng.integers(0, 100, m1).astype(np.int64))],
        {"z": rng.random(m1) < 0.15})
    k0 = (np.arange(m0) + 1).astype(np.int64)               # dense
    b0, b0d, b0n = register(eng, f"pw_x0_{mode}", [
        ("bk", "int64", k0),
        ("x", "int32", rng.integers(0, 100, m0).astype(np.int32)),
        ("nk", "int64", rng.choice(np.concatenate([k1, [1, 2]]), m0))],
        {"x": rng.random(m0) < 0.15})
    t, d, nl = register(eng, f"pw_xd_{mode}", [
        ("fk", "int64", rng.integers(0, m0 + 10, n).astype(np.int64)),
        ("y", "int32", rng.integers(0, 100, n).astype(np.int32)),
        ("g", "char1", rng.integers(0, 4, n).astype(np.uint8))],
        {"y": rng.random(n) < 0.1})
    j0 = join(b0, b0d, b0n, "bk", "fk", kind="inner")
    # a driving column against an INNER payload column
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j0], ["g"],
                         ["count", ("sum", [((0, "x"), "id")])],
                         [("cmp", "y", ">", (0, "x"))])
    _check_paths(paths, mode)
    assert 0 < _count(exp) < n
    # the payloads of two joins, the second chained through the first's
    j1 = join(b1, b1d, b1n, "bk", "nk", kind="left", probe_src=1)
    for where in ([("cmp", (0, "x"), "<=", (1, "z"))],
                  [[("cmp", (0, "x"), "<=", (1, "z")), ("is_null", (1, "z"))],
                   ("not_null", "y")]):
        _p, exp, _paths = run(eng, mode, t, d, nl, [], [j0, j1], ["g"],
                              ["count", ("max", ((1, "z"), "id"))], where)
        assert 0 < _count(exp) < n


# ---- build scope ----

def _build_case(eng, tag, dup_pass=False):
    """build rows whose key 5 occurs twice: the second copy has v = 99 and
    fails `v < 50` unless dup_pass"""
    bk = np.array([1, 2, 3, 4, 5, 5, 6, 7], np.int64)
    v = np.array([10, 60, 20, 70, 30, 30 if dup_pass else 99, 40, 80],
                 np.int32)
    u = np.array([1, 1, 2, 2, 3, 3, 1, 2], np.uint8)
    bt, bd, bn = register(eng, f"pw_bs_b_{tag}", [
        ("bk", "int64", bk), ("v", "int32", v), ("u", "char1", u)],
        {"u": np.array([0, 0, 0, 0, 0, 0, 1, 0], bool)})
    fk = np.array([1, 2, 3, 4, 5, 6, 7, 8, 5, 1, 6], np.int64)
    t, d, nl = register(eng, f"pw_bs_d_{tag}", [
        ("fk", "int64", fk),
        ("y", "int32", np.arange(len(fk)).astype(np.int32))])
    return bt, bd, bn, t, d, nl


@pytest.mark.parametrize("kind", ["semi", "inner", "left", "anti"])
def test_build_scope_on_every_join_kind(eng, mode, kind):
    bt, bd, bn, t, d, nl = _build_case(eng, f"{kind}_{mode}")
    payload = kind in ("inner", "left")
    aggs = ["count"] + ([("count", (0, "v")), ("sum", [((0, "v"), "id")])]
                        if payload else [])
    # duplicates among rows failing the clause compile and run
    bw = [[("range", "v", NEG_INF, 50), ("is_null", "u")],
          ("cmp", "v", ">", "bk")]
    j = wjoin(bt, bd, bn, "bk", "fk", kind=kind, where=bw)
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j], [], aggs)
    _check_paths(paths, mode)
    # partners: keys 1, 3, 5 (first copy), 6 (u NULL); driving hits = 7
    want = {"semi": 7, "inner": 7, "left": 11, "anti": 4}[kind]
    assert exp[0][2][0] == want
    # a clause rejecting every build row
    j = wjoin(bt, bd, bn, "bk", "fk", kind=kind,
              where=[("eq", "v", -1)], preds=[("v", 0, 1000)])
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [j], [], aggs,
                          [("not_null", (0, "v"))] if kind == "left" else ())
    assert exp[0][2][0] == {"semi": 0, "inner": 0, "left": 0, "anti": 11}[kind]


@pytest.mark.parametrize("kind", ["inner", "left"])
def test_build_scope_duplicates_among_passing_rows(eng, mode, kind):
    from greengage_amd import EngineError
    bt, bd, bn, t, d, nl = _build_case(eng, f"dup_{kind}_{mode}", True)
    j = wjoin(bt, bd, bn, "bk", "fk", kind=kind,
              where=[("range", "v", NEG_INF, 50)])
    with plan_mode(mode):
        p = eng.compile_plan(t, joins=strip([j]), aggs=["count"])
        with pytest.raises(EngineError, match="status 5:"):
            eng.execute_plan(p, max_groups=8)


# ---- composition ----

def test_one_column_in_every_role(eng, mode):
    rng = np.random.default_rng(51)
    n = 257
    t, d, nl = register(eng, f"pw_role_{mode}", [
        ("a", "int32", rng.integers(0, 12, n).astype(np.int32)),
        ("b", "int32", rng.integers(0, 12, n).astype(np.int32))],
        {"a": rng.random(n) < 0.1})
    aggs = [("sum", [("a", "id"), ("a", "sub100")]),
            ("filter", "count", [("a", 2, 9)]), ("min", ("a", "id"))]
    _p, exp, paths = run(eng, mode, t, d, nl, [("a", 1, 11)], [], ["a"], aggs,
                         [[("in", "a", [2, 3, 5, 7]), ("cmp", "a", ">", "b")],
                          ("ne", "a", 6)])
    _check_paths(paths, mode)
    assert len(exp) > 3 and all(k0 != 6 for k0, _k1, _v in exp)


def test_where_with_order_and_limit_on_the_device(eng, mode):
    rng = np.random.default_rng(52)
    n, limit = 6001, 5
    t, d, nl = register(eng, f"pw_topk_{mode}", [
        ("k", "int32", rng.integers(0, 300, n).astype(np.int32)),
        ("a", "int64", rng.integers(0, 1000, n).astype(np.int64)),
        ("b", "int64", rng.integers(0, 1000, n).astype(np.int64))])
    where = [[("cmp", "a", "<", "b"), ("in", "k", [1, 2, 3])]]
    aggs = [("sum", [("a", "id")]), "count"]
    by = [("agg", 0, "desc")]
    exp = order_groups(eval_plan(n, d, nl, [], [], ["k"], aggs, where), by,
                       limit)
    with plan_mode(mode):
        p = eng.compile_plan(t, group_cols=["k"], aggs=aggs, where=where,
                             order_by=by, limit=limit)
        for _r in range(3):
            got = eng.execute_plan(p)
            assert [(g[0], g[1], g[2]) for g in got] == exp
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    assert "path_plan_topk_device" in paths and "path_plan_where" in paths


# ---- paths ----

def test_baked_kernel_runs_a_where(eng):
    rng = np.random.default_rng(61)
    n = 6001
    t, d, nl = register(eng, "pw_bake", [
        ("g", "char1", rng.integers(0, 4, n).astype(np.uint8)),
        ("a", "int32", rng.integers(0, 100, n).astype(np.int32)),
        ("b", "int32", rng.integers(0, 100, n).astype(np.int32))])
    p, _exp, paths = run(eng, "rtc", t, d, nl, [], [], ["g"],
                         ["count", ("sum", [("a", "id")])],
                         [[("cmp", "a", "<", "b"), ("eq", "a", 50)]])
    assert paths & {"path_plan_rtc_baked", "path_plan_rtc_baked_fast"}
    by = {s["name"]: s["launches"] for s in eng.stats(p)}
    assert by["path_plan_where"] == 3       # one per execute


def test_no_clause_goes_through_the_old_entry_point(eng, mode, wide):
    t, d, nl = wide
    args = dict(preds=[("p1", -10, 10)], group_cols=["p0"],
                aggs=["count", ("sum", [("p2", "id")])])
    with plan_mode(mode):
        p0 = eng.compile_plan(t, **args)
        p1 = eng.compile_plan(t, where=(), **args)
        assert eng.execute_plan(p0) == eng.execute_plan(p1)
    for p in (p0, p1):
        assert "path_plan_where" not in {s["name"] for s in eng.stats(p)}
    # an extension without clauses through the new entry point: the same
    from greengage_amd import engine as ge
    desc, _k = ge.build_plan_desc(t, **args)
    w, h = ge._PlanWhere(), ctypes.c_int32()
    assert ge.lib().gg_engine_compile_plan_where(
        ctypes.byref(desc), ctypes.byref(w), ctypes.byref(h)) == 0
    assert ge.lib().gg_engine_compile_plan_where(
        ctypes.byref(desc), None, ctypes.byref(h)) == 0


# ---- errors ----

def test_errors(eng):
    from greengage_amd import engine as ge
    rng = np.random.default_rng(71)
    bt, _bd, _bn = register(eng, "pw_err_b", [
        ("bk", "int64", np.arange(5).astype(np.int64)),
        ("d2", "dec64", np.arange(5).astype(np.int64))])
    t, _d, _nl = register(eng, "pw_err_d", [
        ("a", "int64", rng.integers(0, 5, 9).astype(np.int64)),
        ("m", "dec64", rng.integers(0, 5, 9).astype(np.int64))])

    def jn(kind):
        return {"table": bt, "build_key": "bk", "probe_key": "a",
                "kind": kind}

    def status(where=(), joins=(), mutate=None):
        desc, _k = ge.build_plan_desc(t, joins=joins, aggs=["count"])
        w = ge.build_plan_where(joins, where)
        if mutate:
            mutate(w)
        h = ctypes.c_int32()
        return ge.lib().gg_engine_compile_plan_where(
            ctypes.byref(desc), ctypes.byref(w), ctypes.byref(h))

    one = ("eq", "a", 1)

    def setter(path, value):
        def f(w):
            obj = w
            for part in path[:-1]:
                obj = obj[part] if isinstance(part, int) \
                    else getattr(obj, part)
            setattr(obj, path[-1], value)
        return f

    assert status([one]) == 0
    # GG_ENOTSUP: the extension's shape
    assert status([one], mutate=setter(("nclauses",), 9)) == ENOTSUP
    assert status([one], mutate=setter(("nclauses",), -1)) == ENOTSUP
    assert status([one], mutate=setter(("clauses", 0, "natoms"), 9)) == ENOTSUP
    assert status([[one] * 8, [one] * 8], mutate=setter(
        ("nclauses",), 3)) == EINVAL        # clause 2 is empty
    assert status([[one] * 8, [one] * 7, one],
                  mutate=setter(("clauses", 1, "natoms"), 8)) == ENOTSUP
    assert status([one],
                  mutate=setter(("clauses", 0, "atoms", 0, "kind"), 8)) \
        == ENOTSUP
    assert status([one],
                  mutate=setter(("clauses", 0, "atoms", 0, "kind"), -1)) \
        == ENOTSUP
    assert status([("cmp", "a", "<", "m")]) == ENOTSUP      # scales differ
    assert status([("cmp", "m", "<", "m")]) == 0
    assert status([("cmp", (0, "d2"), "=", "m")], [jn("inner")]) == 0
    # GG_EINVAL
    assert status([one], mutate=setter(("clauses", 0, "natoms"), 0)) == EINVAL
    assert status([one], mutate=setter(("clauses", 0, "scope"), 1)) == EINVAL
    assert status([one], mutate=setter(("clauses", 0, "scope"), -1)) == EINVAL
    assert status([("eq", "nope", 1)]) == EINVAL
    assert status([("cmp", "a", "<", "nope")]) == EINVAL
    assert status([one], mutate=setter(
        ("clauses", 0, "atoms", 0, "col2"), b"a")) == EINVAL
    assert status([("cmp", "a", "<", "a")], mutate=setter(
        ("clauses", 0, "atoms", 0, "col2"), None)) == EINVAL
    for kind in ("semi", "anti"):
        assert status([("eq", (0, "bk"), 1)], [jn(kind)]) == EINVAL
    assert status([("eq", (0, "bk"), 1)], [jn("left")]) == 0
    assert status([("eq", (1, "bk"), 1)], [jn("inner")]) == EINVAL
    assert status([("cmp", "a", "<", (1, "bk"))], [jn("inner")]) == EINVAL
    # a build scope reads its own table only
    assert status((), [dict(jn("semi"), where=[("eq", "bk", 1)])]) == 0
    assert status((), [dict(jn("inner"), where=[("eq", (0, "bk"), 1)])]) \
        == EINVAL
    assert status((), [dict(jn("inner"), where=[("eq", "a", 1)])]) == EINVAL
