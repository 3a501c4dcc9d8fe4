"""HAVING of compiled plans (engine_abi.h gg_plan_having).

Reference: plan_having_ref filters the evaluator's groups in Python with big
ints, plan_order_ref orders and limits what is left; every comparison is row
for row and in order.

Every plan is executed on the default path and under GG_PLAN_HAVING=host;
both must give the reference's rows.  The stat rows say which path ran
(one segment and more than 8 groups: the device), plan_having's rows_in /
rows_out must be the group and survivor counts, and under an order exactly
one of path_plan_topk_device / path_plan_topk_host counts per execute: the
device's exactly when the device filtered and more groups survived than the
limit.

The scans run on the interpreted kernel unless a test says otherwise: the
HAVING runs behind the scan whichever kernel it was.
"""
import ctypes
import os

import numpy as np
import pytest

from plan_having_ref import I128_MAX, I128_MIN, filter_groups
from plan_order_ref import order_groups
from plan_payload_ref import join, strip
from plan_where_ref import eval_plan
from plan_outer_ref import plan_mode, register

pytestmark = pytest.mark.gpu

ENOTSUP, EINVAL = 5, 1
SUMX = ("sum", [("x", "id")])


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


def _consts():
    from greengage_amd import PLAN_MAX_LIMIT, plan_topk_tile
    return PLAN_MAX_LIMIT, plan_topk_tile()


def stats_of(eng, p):
    return {s["name"]: s for s in eng.stats(p)}


def stat(eng, p, name, field="launches"):
    s = stats_of(eng, p).get(name)
    return s[field] if s else 0


def _first_diff(got, exp):
    if len(got) != len(exp):
        return ("length", len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        if g != e:
            return (i, g, e)
    return None


class Tab(dict):
    pass


def make_tab(eng, name, cols, nullmap, joins=()):
    """a registered table and a memo of its unfiltered reference results,
    one eval_plan per (group columns, aggregates, where)"""
    t, data, nulls = register(eng, name, cols, nullmap)
    n = len(cols[0][2])
    memo = {}

    def full(group_cols, aggs, where=()):
        k = repr((group_cols, aggs, where))
        if k not in memo:
            memo[k] = eval_plan(n, data, nulls, [], list(joins), group_cols,
                                aggs, where)
        return memo[k]
    return Tab(t=t, full=full, n=n, joins=list(joins))


def run_having(eng, tab, group_cols, aggs, having, order_by=(), limit=0,
               mode="interp", est_groups=0, repeats=1, where=()):
    """Compile with `having`, execute `repeats` times on the default path
    and once under GG_PLAN_HAVING=host; every result must be the
    reference's, in order, and the stat rows must tell the paths.
    Returns (plan, expected rows, number of groups, survivors)."""
    max_limit, _tile = _consts()
    full = tab["full"](group_cols, aggs, where)
    surv = filter_groups(full, having)
    exp = order_groups(surv, order_by, limit)
    ng, ns = len(full), len(surv)
    ordered = bool(order_by) or limit > 0
    device = ng > 8
    topk = device and 0 < limit <= max_limit and ns > limit
    room = max(len(exp), 1)     # the arena holds the emitted rows only
    with plan_mode(mode):
        p = eng.compile_plan(tab["t"], joins=strip(tab["joins"]),
                             group_cols=group_cols, aggs=aggs,
                             order_by=order_by, limit=limit,
                             est_groups=est_groups, where=where,
                             having=having)
        for r in range(repeats):
            got = eng.execute_plan(p, max_groups=room)
            assert got == exp, (r, having, _first_diff(got, exp))
        st = stats_of(eng, p)
        if device:
            assert st["path_plan_having_device"]["launches"] == repeats
            assert "path_plan_having_host" not in st
            assert st["plan_having"]["launches"] == repeats
            assert st["plan_having"]["rows_in"] == repeats * ng
            assert st["plan_having"]["rows_out"] == repeats * ns
        else:
            assert st["path_plan_having_host"]["launches"] == repeats
            assert "path_plan_having_device" not in st
            assert "plan_having" not in st
        tdev = stat(eng, p, "path_plan_topk_device")
        thost = stat(eng, p, "path_plan_topk_host")
        if ordered:
            assert (tdev, thost) == ((repeats, 0) if topk else (0, repeats))
        else:
            assert (tdev, thost) == (0, 0)
        os.environ["GG_PLAN_HAVING"] = "host"
        try:
            got = eng.execute_plan(p, max_groups=room)
        finally:
            del os.environ["GG_PLAN_HAVING"]
        assert got == exp, ("host", having, _first_diff(got, exp))
        assert stat(eng, p, "path_plan_having_host") == (
            1 if device else repeats + 1)
        assert stat(eng, p, "path_plan_having_device") == (
            repeats if device else 0)
        assert stat(eng, p, "plan_having") == (repeats if device else 0)
        if ordered:     # the host's survivors are ordered on the host
            assert stat(eng, p, "path_plan_topk_host") == thost + 1
            assert stat(eng, p, "path_plan_topk_device") == tdev
    return p, exp, ng, ns


def _dup(rng, keys, extra):
    """one row per key plus `extra` duplicate rows, shuffled"""
    rows = np.concatenate([keys, rng.choice(keys, extra)])
    return rows[rng.permutation(len(rows))]


# ---- atoms and aggregate kinds ----

@pytest.fixture(scope="module")
def single(eng):
    """~640 groups by one nullable int64 key; m is NULL on 30% of the rows,
    so that many (mostly one-row) groups have a NULL MIN/MAX"""
    rng = np.random.default_rng(6101)
    keys = (rng.permutation(5000)[:640] * 7919 - 10 ** 7).astype(np.int64)
    k = _dup(rng, keys, 60)
    n = len(k)
    cols = [("k", "int64", k),
            ("x", "int64", rng.integers(-1000, 1000, n).astype(np.int64)),
            ("m", "int32", rng.integers(-50, 50, n).astype(np.int32))]
    nullmap = {"k": rng.random(n) < 0.02, "m": rng.random(n) < 0.3}
    return make_tab(eng, "ph_single", cols, nullmap)


@pytest.fixture(scope="module")
def carry(eng):
    """~500 groups of ~40 rows whose SUM(a*b) passes 2^64, and, b being
    negated for the odd keys, -2^64 as well"""
    from test_gpu_plan_carry import _many_groups
    cols, nullmap, _g = _many_groups()
    cols = dict((c, (t, a)) for c, t, a in cols)
    k, b = cols["k"][1], cols["b"][1]
    cols["b"] = ("int64", np.where(k % 2 == 0, b, -b).astype(np.int64))
    return make_tab(eng, "ph_carry",
                    [(c, t, a) for c, (t, a) in cols.items()], nullmap)


@pytest.fixture(scope="module")
def pair(eng):
    """~900 groups by a packed pair (nullable int32, nullable int64)"""
    rng = np.random.default_rng(6102)
    code = _dup(rng, rng.permutation(40 * 60)[:900], 90)
    n = len(code)
    cols = [("g0", "int32", (code // 60 - 20).astype(np.int32)),
            ("g1", "int64", (code % 60 * 10 ** 6 - 7).astype(np.int64)),
            ("x", "int64", rng.integers(0, 3, n).astype(np.int64))]
    nullmap = {"g0": rng.random(n) < 0.05, "g1": rng.random(n) < 0.05}
    return make_tab(eng, "ph_pair", cols, nullmap)


@pytest.fixture(scope="module")
def chars(eng):
    """~700 groups by two nullable char1 columns, bytes up to 255"""
    rng = np.random.default_rng(6103)
    alpha = np.concatenate([np.arange(0, 15), np.arange(241, 256)])
    code = _dup(rng, rng.permutation(900)[:700], 70)
    n = len(code)
    cols = [("c0", "char1", alpha[code // 30].astype(np.uint8)),
            ("c1", "char1", alpha[code % 30].astype(np.uint8)),
            ("x", "int64", rng.integers(-9, 9, n).astype(np.int64))]
    nullmap = {"c0": rng.random(n) < 0.05, "c1": rng.random(n) < 0.05}
    return make_tab(eng, "ph_chars", cols, nullmap)


def test_having_count_star(eng, single):
    _p, exp, ng, ns = run_having(eng, single, ["k"], ["count", SUMX],
                                 [("cmp", 0, ">=", 2)])
    assert 10 < ns < ng // 4 and all(g[2][0] >= 2 for g in exp)


def test_having_negative_sum(eng, single):
    _p, exp, ng, ns = run_having(eng, single, ["k"], ["count", SUMX],
                                 [("cmp", 1, "<", -500)])
    assert 50 < ns < ng // 2 and all(g[2][1] < -500 for g in exp)
    # a range that straddles zero, and its exact complement
    _p, _e, _ng, inside = run_having(eng, single, ["k"], ["count", SUMX],
                                     [("range", 1, -100, 100)])
    _p, _e, _ng, outside = run_having(eng, single, ["k"], ["count", SUMX],
                                      [("not_range", 1, -100, 100)])
    assert inside > 20 and inside + outside == ng


@pytest.mark.parametrize("side", ["above", "below", "between", "outside"])
def test_having_sum_beyond_two_words(eng, carry, side):
    aggs = [("sum", [("a", "id"), ("b", "id")]), "count"]
    full = carry["full"](["k"], aggs)
    big = 1 << 64
    assert max(g[2][0] for g in full) > big + 1
    assert min(g[2][0] for g in full) < -big - 1
    having = {"above": [("cmp", 0, ">", big + 1)],
              "below": [("cmp", 0, "<=", -big - 1)],
              "between": [("range", 0, -big - 1, big + 1)],
              "outside": [("not_range", 0, -big - 1, big + 1)]}[side]
    _p, _exp, ng, ns = run_having(eng, carry, ["k"], aggs, having,
                                  order_by=[("agg", 0, "desc")], limit=20)
    assert 0 < ns < ng


@pytest.mark.parametrize("kind", ["min", "max"])
def test_having_minmax_with_null_groups(eng, single, kind):
    aggs = [(kind, ("m", "id")), "count"]
    full = single["full"](["k"], aggs)
    nnull = sum(g[2][0] is None for g in full)
    assert 50 < nnull < len(full) - 50
    got = {}
    for name, having in (("range", [("range", 0, -10, 10)]),
                         ("not_range", [("not_range", 0, -10, 10)]),
                         ("is_null", [("is_null", 0)]),
                         ("not_null", [("not_null", 0)]),
                         ("open", [("range", 0, I128_MIN, I128_MAX)]),
                         ("neg", [("cmp", 0, "<", 0)])):
        _p, exp, ng, got[name] = run_having(eng, single, ["k"], aggs, having)
        assert (name == "is_null") == any(g[2][0] is None for g in exp)
    assert got["is_null"] == nnull and got["not_null"] == ng - nnull
    # a comparison over a NULL is not true, either way round
    assert got["range"] + got["not_range"] == ng - nnull == got["open"]
    assert got["range"] > 20 and got["neg"] > 20
    # COUNT is never NULL
    _p, _e, ng, ns = run_having(eng, single, ["k"], aggs, [("is_null", 1)])
    assert ns == 0
    _p, _e, ng, ns = run_having(eng, single, ["k"], aggs, [("not_null", 1)])
    assert ns == ng


def test_having_filtered_count_zero_in_some_groups(eng, single):
    aggs = [("filter", "count", [("x", 0, 1000)]), "count", SUMX]
    full = single["full"](["k"], aggs)
    zeros = sum(g[2][0] == 0 for g in full)
    assert 100 < zeros < len(full) - 100
    _p, _e, _ng, ns = run_having(eng, single, ["k"], aggs,
                                 [("cmp", 0, "=", 0)])
    assert ns == zeros
    _p, _e, ng, ns = run_having(eng, single, ["k"], aggs,
                                [("cmp", 0, ">=", 1)])
    assert ns == ng - zeros


def test_having_or_and_in(eng, single):
    aggs = ["count", SUMX, ("max", ("m", "id"))]
    # SUM(x) < -900 OR MAX(m) IS NULL OR COUNT(*) = 2
    _p, exp, ng, ns = run_having(
        eng, single, ["k"], aggs,
        [[("cmp", 1, "<", -900), ("is_null", 2), ("cmp", 0, "=", 2)]])
    assert 50 < ns < ng
    assert {"sum", "null", "count"} == {
        "sum" if g[2][1] < -900 else "null" if g[2][2] is None else "count"
        for g in exp}
    # two ANDed clauses
    _p, exp, ng, ns = run_having(
        eng, single, ["k"], aggs,
        [("cmp", 1, ">", 0), [("cmp", 2, ">=", 10), ("cmp", 0, ">=", 2)]])
    assert 20 < ns < ng // 2
    # IN over small counts, with an order on top
    _p, exp, ng, ns = run_having(
        eng, single, ["k"], aggs, [("in", 0, [2, 3, 40])],
        order_by=[("agg", 1, "asc")], limit=7)
    assert ns > 7 and {g[2][0] for g in exp} <= {2, 3}


def test_having_packed_pair(eng, pair):
    p, exp, ng, ns = run_having(eng, pair, ["g0", "g1"], ["count", SUMX],
                                [("cmp", 1, ">=", 2)],
                                order_by=[("key", 1, "desc")], limit=30)
    assert "path_plan_group_packed" in stats_of(eng, p)
    assert 30 < ns < ng and len(exp) == 30


def test_having_char_pair(eng, chars):
    p, exp, ng, ns = run_having(eng, chars, ["c0", "c1"], ["count", SUMX],
                                [("not_range", 1, -3, 4)])
    assert "path_plan_group_packed" not in stats_of(eng, p)
    assert 50 < ns < ng
    assert [(g[0], g[1]) for g in exp] == sorted((g[0], g[1]) for g in exp)


def test_having_over_where_and_inner_join(eng):
    rng = np.random.default_rng(6104)
    nd = 50
    dcols = [("dk", "int64", np.arange(nd, dtype=np.int64)),
             ("dv", "int64", rng.integers(-20, 20, nd).astype(np.int64))]
    dt, ddata, dnulls = register(eng, "ph_dim", dcols, {})
    keys = (rng.permutation(3000)[:400] * 13 - 999).astype(np.int64)
    k = _dup(rng, keys, 800)
    n = len(k)
    cols = [("k", "int64", k),
            ("f", "int64", rng.integers(0, 60, n).astype(np.int64)),
            ("x", "int64", rng.integers(-1000, 1000, n).astype(np.int64))]
    tab = make_tab(eng, "ph_fact", cols, {"f": rng.random(n) < 0.05},
                   joins=[join(dt, ddata, dnulls, "dk", "f", kind="inner")])
    aggs = ["count", ("sum", [((0, "dv"), "id")])]
    where = [[("range", "x", -600, 600), ("is_null", "f")]]
    full = tab["full"](["k"], aggs, where)
    assert len(full) < 400         # the join and the WHERE drop whole groups
    p, exp, ng, ns = run_having(eng, tab, ["k"], aggs,
                                [("cmp", 1, ">", 0), ("cmp", 0, ">=", 2)],
                                order_by=[("agg", 1, "desc")], limit=15,
                                where=where)
    assert ns > 15 and "path_plan_where" in stats_of(eng, p)


# ---- the selection's boundaries ----

def _count_tab(eng, ng):
    rng = np.random.default_rng(6200 + ng)
    keys = (rng.permutation(4 * ng)[:ng] * 3 - ng).astype(np.int64)
    k = _dup(rng, keys, max(1, ng // 25))
    cols = [("k", "int64", k),
            ("x", "int64", rng.integers(-10 ** 6, 10 ** 6, len(k)).astype(
                np.int64))]
    return make_tab(eng, f"ph_count_{ng}", cols, {})


_COUNT_TABS = {}


@pytest.fixture(scope="module")
def count_tab(eng):
    def get(ng):
        if ng not in _COUNT_TABS:
            _COUNT_TABS[ng] = _count_tab(eng, ng)
        return _COUNT_TABS[ng]
    yield get
    _COUNT_TABS.clear()


def _thresholds(sums):
    """HAVING clauses over aggregate 0 and the survivors each must leave,
    from the reference's values alone: none, all, exactly one, about half"""
    s = sorted(sums)
    assert s[-1] != s[-2], "the largest sum is unique"
    half = s[len(s) // 2]
    return [([("cmp", 0, ">", s[-1])], 0),
            ([("cmp", 0, ">=", s[0])], len(s)),
            ([("cmp", 0, ">=", s[-1])], 1),
            ([("cmp", 0, ">=", half)], sum(v >= half for v in s))]


NG_OF = {"9": lambda tile: 9, "63": lambda tile: 63, "64": lambda tile: 64,
         "65": lambda tile: 65, "255": lambda tile: 255,
         "256": lambda tile: 256, "257": lambda tile: 257,
         "2*tile+1": lambda tile: 2 * tile + 1}


@pytest.mark.parametrize("groups", list(NG_OF))
def test_selection_boundaries(eng, count_tab, groups):
    _max_limit, tile = _consts()
    ng = NG_OF[groups](tile)
    tab = count_tab(ng)
    full = tab["full"](["k"], [SUMX, "count"])
    assert len(full) == ng
    for having, want in _thresholds([g[2][0] for g in full]):
        assert len(filter_groups(full, having)) == want
        _p, exp, gng, ns = run_having(eng, tab, ["k"], [SUMX, "count"],
                                      having)
        assert (gng, ns, len(exp)) == (ng, want, want)
    assert abs(_thresholds([g[2][0] for g in full])[3][1] - ng / 2) <= 1


NBIG = 2048 * 256 + 257     # one more stride step than pl_grid's clamp gives


@pytest.fixture(scope="module")
def big(eng):
    """2048 * 256 + 257 groups by one int64 key and ~8000 duplicate rows.
    The reference is direct numpy (exact: the sums stay far inside int64),
    the evaluator's per-group Python loop being quadratic"""
    rng = np.random.default_rng(6400)
    keys = (rng.permutation(2 * NBIG)[:NBIG] * 5 - NBIG).astype(np.int64)
    k = _dup(rng, keys, 8000)
    x = rng.integers(-10 ** 9, 10 ** 9, len(k)).astype(np.int64)
    t = eng.register_table("ph_big", [("k", "int64", k), ("x", "int64", x)],
                           len(k))
    uk, inv = np.unique(k, return_inverse=True)
    sums = np.zeros(len(uk), np.int64)
    np.add.at(sums, inv, x)
    cnts = np.bincount(inv, minlength=len(uk)).astype(np.int64)
    assert len(uk) == NBIG
    return t, uk, sums, cnts


def _arena_rows(raw, nslots):
    """a raw arena as (n_groups, int64 array of n_groups x (2 + 2 * nslots))"""
    ng = int.from_bytes(raw[0:8], "little", signed=True)
    assert int.from_bytes(raw[8:12], "little") == nslots
    w = 2 + 2 * nslots
    assert len(raw) == 16 + ng * w * 8
    return ng, np.frombuffer(raw, np.int64, ng * w, 16).reshape(ng, w)


@pytest.mark.parametrize("case", ["none", "all", "one", "half", "count>=2"])
def test_selection_past_the_grid_clamp(eng, big, case):
    """every block takes a second stride step, the last a partial one; the
    survivors come back in key order, compared as whole numpy arrays"""
    t, uk, sums, cnts = big
    s = np.sort(sums)
    assert s[-1] != s[-2]
    having, mask = {
        "none": ([("cmp", 0, ">", int(s[-1]))], sums > s[-1]),
        "all": ([("cmp", 0, ">=", int(s[0]))], sums >= s[0]),
        "one": ([("cmp", 0, ">=", int(s[-1]))], sums >= s[-1]),
        "half": ([("cmp", 0, ">=", int(s[NBIG // 2]))],
                 sums >= s[NBIG // 2]),
        "count>=2": ([("cmp", 1, ">=", 2)], cnts >= 2)}[case]
    want = int(mask.sum())
    assert want == {"none": 0, "all": NBIG, "one": 1}.get(case, want)
    if case == "half":
        assert abs(want - NBIG / 2) <= 1
    if case == "count>=2":
        assert 7000 < want < 8000
    exp = np.stack([uk[mask], np.zeros(want, np.int64), sums[mask],
                    sums[mask] >> 63, cnts[mask],
                    np.zeros(want, np.int64)], axis=1)
    size = 16 + want * 48
    with plan_mode("interp"):
        p = eng.compile_plan(t, group_cols=["k"], aggs=[SUMX, "count"],
                             est_groups=NBIG, having=having)
        for path in ("device", "host"):
            if path == "host":
                os.environ["GG_PLAN_HAVING"] = "host"
            try:
                ng, rows = _arena_rows(eng.execute_raw(p, size), 2)
            finally:
                os.environ.pop("GG_PLAN_HAVING", None)
            assert ng == want and np.array_equal(rows, exp), path
    st = stats_of(eng, p)
    assert st["path_plan_having_device"]["launches"] == 1
    assert st["path_plan_having_host"]["launches"] == 1
    assert (st["plan_having"]["rows_in"], st["plan_having"]["rows_out"]) == (
        NBIG, want)
    assert "path_plan_group_grow" not in st


def test_topk_over_survivors_past_the_grid_clamp(eng, big):
    """TPC-H Q18's inner block in small: ~7,700 of 524,545 groups pass, the
    top 100 of them by the sum come back, two tournament rounds over the
    survivor list"""
    t, uk, sums, cnts = big
    _max_limit, tile = _consts()
    mask = cnts >= 2
    surv = [(int(a), 0, [int(s), int(c)])
            for a, s, c in zip(uk[mask], sums[mask], cnts[mask])]
    by, limit = [("agg", 0, "desc")], 100
    exp = order_groups(surv, by, limit)
    with plan_mode("interp"):
        p = eng.compile_plan(t, group_cols=["k"], aggs=[SUMX, "count"],
                             order_by=by, limit=limit, est_groups=NBIG,
                             having=[("cmp", 1, ">=", 2)])
        assert eng.execute_plan(p) == exp
    st = stats_of(eng, p)
    assert st["path_plan_topk_device"]["launches"] == 1
    assert st["plan_topk"]["rows_in"] == len(surv) > 3 * tile
    assert st["plan_topk"]["launches"] == 2
    os.environ["GG_PLAN_HAVING"] = "host"
    try:
        assert eng.execute_plan(p) == exp
    finally:
        del os.environ["GG_PLAN_HAVING"]
    assert stat(eng, p, "path_plan_topk_host") == 1


# ---- with ORDER BY / LIMIT ----

@pytest.fixture(scope="module")
def distinct(eng):
    """2 * tile + 300 one-row groups with distinct x: SUM(x) >= the s-th
    largest x leaves exactly s groups"""
    _max_limit, tile = _consts()
    ng = 2 * tile + 300
    rng = np.random.default_rng(6500)
    k = (rng.permutation(3 * ng)[:ng] * 11 - 5 * ng).astype(np.int64)
    x = (rng.permutation(4 * ng)[:ng] * 17 - 30 * ng).astype(np.int64)
    return make_tab(eng, "ph_distinct", [("k", "int64", k),
                                         ("x", "int64", x)], {})


@pytest.mark.parametrize("survivors", ["limit-1", "limit", "limit+1",
                                       "2*tile+1", "0"])
def test_limit_over_survivors(eng, distinct, survivors):
    _max_limit, tile = _consts()
    limit = 10
    want = {"limit-1": limit - 1, "limit": limit, "limit+1": limit + 1,
            "2*tile+1": 2 * tile + 1, "0": 0}[survivors]
    aggs = [SUMX, "count"]
    full = distinct["full"](["k"], aggs)
    desc = sorted((g[2][0] for g in full), reverse=True)
    having = ([("cmp", 0, ">=", desc[want - 1])] if want
              else [("cmp", 0, ">", desc[0])])
    assert len(filter_groups(full, having)) == want
    # ascending: the head of the result is the survivors' tail
    p, exp, _ng, ns = run_having(eng, distinct, ["k"], aggs, having,
                                 order_by=[("agg", 0, "asc")], limit=limit)
    assert ns == want and len(exp) == min(want, limit)
    # run_having asserted the top-k rows; the device's count is survivors >
    # limit exactly
    assert stat(eng, p, "path_plan_topk_device") == (1 if want > limit else 0)
    if want > limit:
        st = stats_of(eng, p)["plan_topk"]
        assert st["rows_in"] == want
        assert st["launches"] == (2 if want > tile else 1)
        assert exp[0][2][0] == desc[want - 1]


def test_limit_above_device_cap_over_survivors(eng, distinct):
    max_limit, tile = _consts()
    aggs = [SUMX, "count"]
    full = distinct["full"](["k"], aggs)
    desc = sorted((g[2][0] for g in full), reverse=True)
    p, exp, _ng, ns = run_having(eng, distinct, ["k"], aggs,
                                 [("cmp", 0, ">=", desc[max_limit + 49])],
                                 order_by=[("agg", 0, "desc")],
                                 limit=max_limit + 1)
    assert ns == max_limit + 50 and len(exp) == max_limit + 1
    assert stat(eng, p, "path_plan_topk_device") == 0
    # and an order without a limit returns every survivor, ordered
    _p, exp, _ng, ns = run_having(eng, distinct, ["k"], aggs,
                                  [("cmp", 0, ">=", desc[99])],
                                  order_by=[("agg", 0, "asc")])
    assert ns == 100 and [g[2][0] for g in exp] == desc[99::-1]


# ---- the host path, the bake, ngroup == 0, the arena ----

def test_up_to_eight_groups_go_to_the_host(eng, count_tab):
    for ng in (8, 1):
        tab = count_tab(ng)
        full = tab["full"](["k"], [SUMX, "count"])
        s = sorted(g[2][0] for g in full)
        p, _exp, gng, ns = run_having(eng, tab, ["k"], [SUMX, "count"],
                                      [("cmp", 0, ">=", s[ng // 2])],
                                      order_by=[("agg", 0, "desc")], limit=3)
        assert gng == ng and ns == ng - ng // 2
        assert "path_plan_having_device" not in stats_of(eng, p)


def test_host_having_bakes_from_the_full_group_set(eng):
    """4 groups: the HAVING runs on the host behind the bake, which keeps
    its whole group set, so the baked executes still find every group and
    come out filtered like the first"""
    rng = np.random.default_rng(6300)
    n = 3000
    cols = [("c0", "char1", rng.choice(np.frombuffer(b"AN", np.uint8), n)),
            ("c1", "char1", rng.choice(np.frombuffer(b"FO", np.uint8), n)),
            ("x", "int64", rng.integers(-50, 100, n).astype(np.int64))]
    tab = make_tab(eng, "ph_baked", cols, {})
    full = tab["full"](["c0", "c1"], [SUMX, "count"])
    s = sorted(g[2][0] for g in full)
    assert len(s) == 4 and s[1] != s[2]
    p, exp, ng, ns = run_having(eng, tab, ["c0", "c1"], [SUMX, "count"],
                                [("cmp", 0, ">=", s[2])], mode="rtc",
                                repeats=3)
    assert (ng, ns, len(exp)) == (4, 2, 2)
    st = stats_of(eng, p)
    assert {"path_plan_rtc_baked", "path_plan_rtc_baked_fast"} & set(st)
    assert "path_plan_bake_miss" not in st
    assert st["path_plan_having_host"]["launches"] == 4


def test_plain_aggregate_row_is_emitted_iff_it_passes(eng, single):
    n = single["n"]
    p, exp, ng, ns = run_having(eng, single, [], ["count", SUMX],
                                [("cmp", 0, "=", n)])
    assert (ng, ns) == (1, 1) and exp[0][2][0] == n
    p, exp, ng, ns = run_having(eng, single, [], ["count", SUMX],
                                [("cmp", 0, ">", n)])
    assert (ng, ns, exp) == (1, 0, [])
    raw = eng.execute_raw(p, 16)
    assert len(raw) == 16       # written == 16: a valid, empty result
    assert int.from_bytes(raw[0:8], "little", signed=True) == 0
    assert int.from_bytes(raw[8:12], "little") == 2
    assert int.from_bytes(raw[12:16], "little") == 0


@pytest.mark.parametrize("path", ["device", "host"])
def test_arena_holds_exactly_the_survivors(eng, single, path):
    from greengage_amd import EngineError
    aggs = ["count", SUMX, ("avg", [("x", "id")])]      # 4 slots a row
    having = [("cmp", 0, ">=", 2)]
    ns = len(filter_groups(single["full"](["k"], aggs), having))
    assert ns > 10
    size = 16 + ns * (16 + 16 * 4)
    with plan_mode("interp"):
        p = eng.compile_plan(single["t"], group_cols=["k"], aggs=aggs,
                             having=having)
        if path == "host":
            os.environ["GG_PLAN_HAVING"] = "host"
        try:
            raw = eng.execute_raw(p, size)
            assert len(raw) == size
            assert int.from_bytes(raw[0:8], "little", signed=True) == ns
            with pytest.raises(EngineError, match="status 1.*arena"):
                eng.execute_raw(p, size - 1)
        finally:
            os.environ.pop("GG_PLAN_HAVING", None)
    assert stat(eng, p, "path_plan_having_" + path) == 2


# ---- compile errors and the no-clause case ----

def test_compile_errors(eng, single):
    from greengage_amd import engine as ge
    t = single["t"]
    aggs = ["count", SUMX, ("avg", [("x", "id")])]

    def status(having=(("cmp", 0, ">", 1),), edit=None, desc_edit=None,
               where=None):
        d = ge.build_plan_desc(t, group_cols=["k"], aggs=aggs)[0]
        if desc_edit:
            desc_edit(d)
        hv = ge.build_plan_having(aggs, list(having))
        if edit:
            edit(hv)
        h = ctypes.c_int32()
        return ge.lib().gg_engine_compile_plan_having(
            ctypes.byref(d), ctypes.byref(where) if where else None,
            ctypes.byref(hv), ctypes.byref(h))

    def clause0(**kw):
        def edit(hv):
            for k, v in kw.items():
                setattr(hv.clauses[0], k, v)
        return edit

    def atom0(**kw):
        def edit(hv):
            for k, v in kw.items():
                setattr(hv.clauses[0].atoms[0], k, v)
        return edit

    def nclauses(v):
        def edit(hv):
            hv.nclauses = v
        return edit

    one = ("cmp", 0, ">", 1)
    assert status() == 0
    assert status([[one] * 4, [one] * 4]) == 0
    # GG_ENOTSUP
    assert status(edit=nclauses(ge.PLAN_MAX_HAVING_CLAUSES + 1)) == ENOTSUP
    assert status(edit=nclauses(-1)) == ENOTSUP
    assert status(edit=clause0(
        natoms=ge.PLAN_MAX_HAVING_ATOMS + 1)) == ENOTSUP

    def nine(hv):                  # 3 + 3 + 3 atoms, each within bounds
        hv.clauses[2].natoms = 3
    assert status([[one] * 3, [one] * 3, [one] * 2], edit=nine) == ENOTSUP
    assert status(edit=atom0(kind=4)) == ENOTSUP
    assert status(edit=atom0(kind=-1)) == ENOTSUP
    assert status(edit=atom0(agg=2)) == ENOTSUP            # the AVG
    # GG_EINVAL
    assert status(edit=clause0(natoms=0)) == EINVAL
    assert status(edit=clause0(natoms=-1)) == EINVAL
    assert status(edit=atom0(agg=3)) == EINVAL
    assert status(edit=atom0(agg=-1)) == EINVAL
    ge.lib().gg_engine_last_error.restype = ctypes.c_char_p
    assert b"having clause" in ge.lib().gg_engine_last_error()

    # the descriptor and the WHERE are validated first
    def bad_limit(d):
        d.limit = -1
    assert status(edit=clause0(natoms=0), desc_edit=bad_limit) == ENOTSUP
    w = ge.build_plan_where((), [("eq", "x", 1)])
    w.clauses[0].natoms = 0
    assert status(edit=nclauses(9), where=w) == EINVAL
    assert b"where clause" in ge.lib().gg_engine_last_error()


def test_no_clause_is_compile_plan_where(eng, single):
    from greengage_amd import engine as ge
    t = single["t"]
    aggs = ["count", SUMX]
    where = [("range", "x", -500, 500)]
    exp = single["full"](["k"], aggs, where)
    with plan_mode("interp"):
        plans = [eng.compile_plan(t, group_cols=["k"], aggs=aggs,
                                  where=where),
                 eng.compile_plan(t, group_cols=["k"], aggs=aggs,
                                  where=where, having=())]
        d = ge.build_plan_desc(t, group_cols=["k"], aggs=aggs)[0]
        w = ge.build_plan_where((), where)
        for hv in (None, ge._PlanHaving()):
            h = ctypes.c_int32()
            assert ge.lib().gg_engine_compile_plan_having(
                ctypes.byref(d), ctypes.byref(w),
                ctypes.byref(hv) if hv is not None else None,
                ctypes.byref(h)) == 0
            plans.append(h.value)
        names = []
        for p in plans:
            assert eng.execute_plan(p) == exp
            names.append(sorted(stats_of(eng, p)))
    assert all(n == names[0] for n in names)
    assert not [n for n in names[0] if "having" in n]
