"""COUNT(DISTINCT) of compiled plans (engine_abi.h GG_AGG_COUNT_DISTINCT).

Reference: plan_distinct_ref evaluates the descriptor directly (Python sets
over the surviving rows), plan_having_ref and plan_order_ref filter and order
its groups; every comparison is row for row and in order.

Every plan is executed three times on the default path and once under
GG_PLAN_DISTINCT=host, on the generated scan and on the interpreted one.
Every execute's stat rows are asserted: which of path_plan_distinct_device /
path_plan_distinct_host counted (one segment and more than 8 (group key,
value) pairs: the device's), and plan_regroup's rows_in / rows_out, which
must be the reference's pair and group counts.
"""
import os

import numpy as np
import pytest

from plan_distinct_ref import (NULL_KEY, eval_plan, pair_count, plan_mode,
                               register, strip)
from plan_having_ref import filter_groups
from plan_order_ref import order_groups
from plan_payload_ref import join

pytestmark = pytest.mark.gpu

ENOTSUP, EINVAL = 5, 1
CDX = ("count_distinct", "x")
MODES = ["rtc", "interp"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


def stats_of(eng, p):
    return {s["name"]: s for s in eng.stats(p)}


def stat(st, name, field="launches"):
    return st[name][field] if name in st else 0


def _first_diff(got, exp):
    if len(got) != len(exp):
        return ("length", len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        if g != e:
            return (i, g, e)
    return None


def make_tab(eng, name, cols, nullmap, joins=()):
    """a registered table and a memo of its reference results: (groups,
    pairs) per (group columns, aggregates)"""
    t, data, nulls = register(eng, name, cols, nullmap)
    n = len(cols[0][2])
    memo = {}

    def full(group_cols, aggs):
        k = repr((group_cols, aggs))
        if k not in memo:
            args = (n, data, nulls, [], list(joins), group_cols, aggs)
            memo[k] = (eval_plan(*args), pair_count(*args))
        return memo[k]
    return dict(t=t, full=full, n=n, joins=list(joins))


def run_distinct(eng, tab, group_cols, aggs, mode, having=(), order_by=(),
                 limit=0, est_groups=0, exp_full=None, npairs=None):
    """Compile, execute three times on the default path and once under
    GG_PLAN_DISTINCT=host; every result must be the reference's, in order,
    and every execute's stat rows must tell the path and the fold's counts.
    Returns (plan, expected rows, groups, pairs, stat rows)."""
    if exp_full is None:
        exp_full, npairs = tab["full"](group_cols, aggs)
    surv = filter_groups(exp_full, having)
    exp = order_groups(surv, order_by, limit)
    ng, ns = len(exp_full), len(surv)
    device = npairs > 8
    room = max(len(exp), 1)
    with plan_mode(mode):
        p = eng.compile_plan(tab["t"], joins=strip(tab["joins"]),
                             group_cols=group_cols, aggs=aggs,
                             order_by=order_by, limit=limit,
                             est_groups=est_groups, having=having)
        for r in range(1, 4):
            got = eng.execute_plan(p, max_groups=room)
            assert got == exp, (mode, r, _first_diff(got, exp))
            st = stats_of(eng, p)
            assert (stat(st, "path_plan_distinct_device"),
                    stat(st, "path_plan_distinct_host")) == (
                (r, 0) if device else (0, r))
            assert stat(st, "plan_regroup") == r
            assert stat(st, "plan_regroup", "rows_in") == r * npairs
            assert stat(st, "plan_regroup", "rows_out") == r * ng
        os.environ["GG_PLAN_DISTINCT"] = "host"
        try:
            got = eng.execute_plan(p, max_groups=room)
        finally:
            del os.environ["GG_PLAN_DISTINCT"]
        assert got == exp, (mode, "host", _first_diff(got, exp))
        st = stats_of(eng, p)
        assert (stat(st, "path_plan_distinct_device"),
                stat(st, "path_plan_distinct_host")) == (
            (3, 1) if device else (0, 4))
        assert stat(st, "plan_regroup", "rows_in") == 4 * npairs
        assert stat(st, "plan_regroup", "rows_out") == 4 * ng
        # behind the fold: the device HAVING and top-k see the plan's own
        # groups on the default path; the host's regroup leaves both to the
        # host.  Exactly one row of each pair counts per execute
        hdev = device and ng > 8
        tdev = hdev and 0 < limit < ns
        if having:
            assert (stat(st, "path_plan_having_device"),
                    stat(st, "path_plan_having_host")) == (
                (3, 1) if hdev else (0, 4))
        if order_by or limit:
            assert (stat(st, "path_plan_topk_device"),
                    stat(st, "path_plan_topk_host")) == (
                (3, 1) if tdev else (0, 4))
        assert (("path_plan_interp" if mode == "interp" else "path_plan_rtc")
                in st)
    return p, exp, ng, npairs, st


# ---- the tables ----

NFLAT = 5000
ALL_NULL_KEY = 777          # the g250 group whose x is NULL on every row


@pytest.fixture(scope="module")
def flat(eng):
    """5000 rows: x has ~300 values and 10% NULLs, w ~700 values; g3 makes
    3 groups, g250 about 250 (int64, negative ones and a NULL group
    included), one of which has only NULL x.  SUM(y * z) passes 2^64 in the
    large groups, with either sign"""
    rng = np.random.default_rng(7301)
    n = NFLAT
    keys = np.concatenate([(rng.permutation(4000)[:249] * 1009 - 2 * 10 ** 6),
                           [ALL_NULL_KEY]]).astype(np.int64)
    g250 = rng.choice(keys, n)
    xn = (rng.random(n) < 0.1) | (g250 == ALL_NULL_KEY)
    cols = [("x", "int64", (rng.integers(0, 300, n) * 37 - 4000).astype(
                np.int64)),
            ("w", "int32", rng.integers(-350, 350, n).astype(np.int32)),
            ("g3", "int32", rng.integers(-1, 2, n).astype(np.int32)),
            ("g250", "int64", g250),
            ("y", "int64", rng.integers(-3 * 10 ** 9, 3 * 10 ** 9, n).astype(
                np.int64)),
            ("z", "int64", rng.integers(1, 3 * 10 ** 9, n).astype(np.int64)),
            ("m", "int32", rng.integers(-50, 50, n).astype(np.int32)),
            ("f", "int64", rng.integers(0, 10, n).astype(np.int64))]
    nullmap = {"x": xn, "g250": rng.random(n) < 0.02,
               "m": rng.random(n) < 0.3}
    return make_tab(eng, "pd_flat", cols, nullmap)


@pytest.mark.parametrize("mode", MODES)
def test_no_group_column(eng, flat, mode):
    """shape 1: every pair folds into one cache slot of every block"""
    _p, exp, ng, npairs, _st = run_distinct(eng, flat, [], [CDX, "count"],
                                            mode)
    assert ng == 1 and npairs == 301 and exp[0][2] == [300, NFLAT]


@pytest.mark.parametrize("mode", MODES)
def test_three_groups_cache_absorbs_everything(eng, flat, mode):
    """shape 2: 3 groups, ~2000 pairs in 8 blocks; the replicas fold"""
    _p, exp, ng, npairs, _st = run_distinct(
        eng, flat, ["g3"], [("count_distinct", "w"), "count"], mode)
    assert ng == 3 and 1800 < npairs <= 2100
    assert all(600 < g[2][0] <= 700 for g in exp)


@pytest.mark.parametrize("mode", MODES)
def test_many_groups_cache_overflows(eng, flat, mode):
    """shapes 3 and 5: 251 groups and > 4000 pairs, so every block's 32
    cache slots overflow into the global table, where cached and uncached
    contributions to one group meet; one group has only NULL values"""
    _p, exp, ng, npairs, _st = run_distinct(
        eng, flat, ["g250"], [CDX, "count", ("count", "x")], mode)
    assert ng == 251 and npairs > 4000 and exp[0][0] == NULL_KEY
    empty = [g for g in exp if g[0] == ALL_NULL_KEY]
    assert len(empty) == 1 and empty[0][2][0] == 0 and empty[0][2][2] == 0
    assert empty[0][2][1] > 5


AGGS8 = [CDX, ("filter", CDX, [("f", 0, 3)]),
         ("sum", [("y", "id"), ("z", "id")]), ("min", ("m", "id")),
         ("max", ("m", "id")), ("avg", [("y", "id")])]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group", ["g3", "g250"])
def test_every_kind_through_the_fold(eng, flat, mode, group):
    """shape 6: two DISTINCT aggregates over one column, one filtered,
    beside SUM, MIN, MAX and AVG: all 8 accumulator slots, kinds 3 and 4
    and the helper counts folded, a negative SUM and one past 2^64"""
    _p, exp, _ng, _np, _st = run_distinct(eng, flat, [group], AGGS8, mode)
    sums = [g[2][2] for g in exp]
    assert min(sums) < 0
    if group == "g3":
        assert max(abs(s) for s in sums) > 1 << 64
    assert all(g[2][1] <= g[2][0] for g in exp)
    assert any(0 < g[2][1] < g[2][0] for g in exp)


@pytest.mark.parametrize("mode", MODES)
def test_having_and_topk_behind_the_fold(eng, flat, mode):
    """shape 9: HAVING on the distinct count and ORDER BY it DESC LIMIT 5
    over 251 groups: the device HAVING and the device top-k both run on the
    regrouped rows (run_distinct asserts their path rows)"""
    _p, exp, ng, _np, st = run_distinct(
        eng, flat, ["g250"], [CDX, "count"], mode,
        having=[("cmp", 0, ">=", 15)],
        order_by=[("agg", 0, "desc"), ("key", 0, "desc")], limit=5)
    assert len(exp) == 5 and exp[0][2][0] >= exp[4][2][0] >= 15
    assert stat(st, "plan_having", "rows_in") == 3 * ng
    assert 5 < stat(st, "plan_having", "rows_out") // 3 < ng
    assert stat(st, "plan_topk") > 0


@pytest.mark.parametrize("mode", MODES)
def test_a_handful_of_pairs_takes_the_host_and_the_bake(eng, mode):
    """shape 4: 8 pairs in all, so the host folds them and bakes the inner
    group set; the second and third executes run the baked inner kernel"""
    g = np.array([1, 1, 1, 2, 2, 2, 2, 1, 3, 3, 2], np.int64)
    x = np.array([5, 5, 6, 5, 0, 7, 7, 0, 0, 0, 9], np.int64)
    tab = make_tab(eng, f"pd_tiny_{mode}",
                   [("g", "int64", g), ("x", "int64", x)], {"x": x == 0})
    _p, exp, ng, npairs, st = run_distinct(eng, tab, ["g"], [CDX, "count"],
                                           mode)
    assert exp == [(1, 0, [2, 4]), (2, 0, [3, 5]), (3, 0, [0, 2])]
    assert (ng, npairs) == (3, 8)
    baked = "path_plan_rtc_baked" in st or "path_plan_rtc_baked_fast" in st
    assert baked == (mode == "rtc")
    assert "path_plan_bake_miss" not in st


@pytest.mark.parametrize("mode", MODES)
def test_empty_input_yields_the_one_row(eng, flat, mode):
    """no group column and no surviving row: one row, every count 0"""
    with plan_mode(mode):
        p = eng.compile_plan(flat["t"], preds=[("f", 100, 200)],
                             aggs=[CDX, "count"])
        for _ in range(3):
            assert eng.execute_plan(p) == [(0, 0, [0, 0])]
    st = stats_of(eng, p)
    assert stat(st, "path_plan_distinct_host") == 3
    assert (stat(st, "plan_regroup", "rows_in"),
            stat(st, "plan_regroup", "rows_out")) == (0, 3)


@pytest.fixture(scope="module")
def joined(eng):
    """shape 7: the distinct column is the payload of a LEFT join that
    leaves about a third of the rows without a partner, the group column
    the payload of an INNER join"""
    rng = np.random.default_rng(7302)
    n, nb, nc = 4000, 400, 60
    bcols = [("bk", "int64", (np.arange(nb) * 3 + 1).astype(np.int64)),
             ("p", "int32", rng.integers(-90, 90, nb).astype(np.int32))]
    ccols = [("ck", "int64", (rng.permutation(500)[:nc] + 1).astype(np.int64)),
             ("grp", "int64", (rng.integers(0, 20, nc) * 10 ** 9).astype(
                 np.int64))]
    bt, bdata, bnulls = register(eng, "pd_b", bcols,
                                 {"p": rng.random(nb) < 0.1})
    ct, cdata, cnulls = register(eng, "pd_c", ccols,
                                 {"grp": rng.random(nc) < 0.1})
    fk = rng.choice(bcols[0][2], n) + (rng.random(n) < 0.33)
    dcols = [("fk", "int64", fk.astype(np.int64)),
             ("ck", "int64", rng.choice(ccols[0][2], n)),
             ("v", "int64", rng.integers(-5, 5, n).astype(np.int64))]
    joins = [join(bt, bdata, bnulls, "bk", "fk", kind="left"),
             join(ct, cdata, cnulls, "ck", "ck", kind="inner")]
    return make_tab(eng, "pd_d", dcols, {"fk": rng.random(n) < 0.05}, joins)


@pytest.mark.parametrize("mode", MODES)
def test_payload_columns_of_left_and_inner_joins(eng, joined, mode):
    aggs = [("count_distinct", (0, "p")), "count", ("count", (0, "p")),
            ("sum", [("v", "id")])]
    _p, exp, ng, npairs, st = run_distinct(eng, joined, [(1, "grp")], aggs,
                                           mode)
    assert ng > 10 and npairs > 8 * ng and exp[0][0] == NULL_KEY
    # partnerless and NULL-payload rows are in COUNT(*) and nowhere else
    assert all(g[2][2] < g[2][1] and 0 < g[2][0] <= g[2][2] for g in exp)
    assert "path_plan_join_left" in st


@pytest.mark.parametrize("mode", MODES)
def test_two_char1_columns_keep_their_code(eng, mode):
    """shape 8: group and distinct column both char1, bytes up to 255 and
    NULLs in both: the inner code is e0 * 512 + e1, not a packed pair"""
    rng = np.random.default_rng(7303)
    n = 3000
    alpha = np.concatenate([np.arange(0, 12), np.arange(244, 256)])
    cols = [("c0", "char1", rng.choice(alpha, n).astype(np.uint8)),
            ("c1", "char1", rng.choice(alpha, n).astype(np.uint8)),
            ("v", "int64", rng.integers(0, 9, n).astype(np.int64))]
    tab = make_tab(eng, f"pd_chars_{mode}", cols,
                   {"c0": rng.random(n) < 0.05, "c1": rng.random(n) < 0.05})
    _p, exp, ng, npairs, st = run_distinct(
        eng, tab, ["c0"], [("count_distinct", "c1"), "count"], mode)
    assert ng == 25 and npairs > 500 and exp[0][0] == NULL_KEY
    assert all(18 <= g[2][0] <= 24 for g in exp)
    assert max(g[2][0] for g in exp) == 24
    assert "path_plan_group_packed" not in st
    # and as the one group column of the inner plan
    run_distinct(eng, tab, [], [("count_distinct", "c1")], mode)


NGROW = 270_000


def test_underestimate_regrows_the_inner_table_once(eng):
    """shape 10: est_groups far below the 270,000 pairs starts the inner
    table on its fixed 2^18 slots, which fill; the scan is redone once on a
    larger table and the result is what the well-estimated plan gives.  The
    reference is direct numpy at this size"""
    rng = np.random.default_rng(7304)
    vals = (rng.permutation(2 * NGROW)[:NGROW] * 5 - NGROW).astype(np.int64)
    x = np.concatenate([vals, rng.choice(vals, 8000)])
    x = x[rng.permutation(len(x))]
    nl = rng.random(len(x)) < 0.01
    t = eng.register_table("pd_grow", [("x", "int64", x)], len(x))
    eng.set_nulls(t, "x", nl.astype(np.uint8))
    exp = [(0, 0, [len(np.unique(x[~nl])), len(x)])]
    npairs = exp[0][2][0] + 1
    tab = dict(t=t, joins=[])
    for est, grows in ((1, 1), (300_000, 0)):
        _p, _e, _ng, _np, st = run_distinct(
            eng, tab, [], [CDX, "count"], "rtc", est_groups=est,
            exp_full=exp, npairs=npairs)
        assert stat(st, "path_plan_group_grow") == grows


# ---- errors ----

def _refused(eng, status, match, t, **kw):
    from greengage_amd import EngineError
    with pytest.raises(EngineError, match=match) as ei:
        eng.compile_plan(t, **kw)
    assert f"status {status}:" in str(ei.value)


def test_compile_time_limits(eng, flat):
    t = flat["t"]
    _refused(eng, ENOTSUP, "two group columns", t, group_cols=["g3", "g250"],
             aggs=[CDX])
    _refused(eng, ENOTSUP, "more than one column", t, group_cols=["g3"],
             aggs=[CDX, ("count_distinct", "w")])
    _refused(eng, ENOTSUP, "exactly one column", t, group_cols=["g3"],
             aggs=[("count_distinct", [("x", "id"), ("w", "id")])])
    _refused(eng, ENOTSUP, "factor mod", t, group_cols=["g3"],
             aggs=[("count_distinct", [("x", "sub100")])])
    _refused(eng, EINVAL, "column missing", t, aggs=[("count_distinct", "no")])
    # the same column counted under two filters is one column
    p = eng.compile_plan(t, group_cols=["g3"], aggs=[
        ("filter", CDX, [("f", 0, 3)]), ("filter", CDX, [("f", 3, 6)]), CDX])
    assert len(eng.execute_plan(p)) == 3


def test_pair_over_62_bits_is_refused_at_the_first_execute(eng):
    from greengage_amd import EngineError
    g = np.array([0, 1 << 40, 5], np.int64)
    x = np.array([-(1 << 40), 7, 1 << 39], np.int64)
    t = eng.register_table("pd_wide", [("g", "int64", g), ("x", "int64", x)],
                           3)
    p = eng.compile_plan(t, group_cols=["g"], aggs=[CDX])
    for _ in range(2):
        with pytest.raises(EngineError, match="the packed code holds 62") \
                as ei:
            eng.execute_plan(p)
        assert f"status {ENOTSUP}:" in str(ei.value)
    # either column alone is fine
    p = eng.compile_plan(t, aggs=[CDX])
    assert eng.execute_plan(p) == [(0, 0, [3])]
