"""ORDER BY / LIMIT and the growable group table of compiled plans
(engine_abi.h gg_plan_order, gg_plan_desc.limit / est_groups).

Reference: plan_order_ref, which sorts plan_outer_ref.eval_plan's groups in
Python with big ints; every comparison is row for row and in order.  Tables
hold about one row per group plus a few percent of duplicates, so that
counts and sums differ between groups while most groups still tie on COUNT.

Every plan with a limit the device top-k serves (one segment, 0 < limit <=
PLAN_MAX_LIMIT, more than max(limit, 8) groups) is also executed under
GG_PLAN_TOPK=host, and both paths must give the reference's rows; the stat
rows tell which path ran.

The scans run on the interpreted kernel unless a test says otherwise: what
orders the groups runs behind the scan whichever kernel it was, and the
interpreted kernel needs no hipRTC compile per plan.
"""
import ctypes
import os

import numpy as np
import pytest

from plan_order_ref import NULL_KEY, eval_plan, order_groups
from plan_outer_ref import plan_mode, register

pytestmark = pytest.mark.gpu

ENOTSUP, EINVAL = 5, 1


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


def launches(eng, p, name):
    s = stats_of(eng, p).get(name)
    return s["launches"] if s else 0


def run_ordered(eng, tab, group_cols, aggs, order_by, limit, mode="interp",
                est_groups=0, repeats=1):
    """Compile, execute `repeats` times on the default path and once under
    GG_PLAN_TOPK=host; every result must be the reference's, in order.
    Returns (plan, expected, device executes, host executes)."""
    t, full = tab["t"], tab["full"](group_cols, aggs)
    exp = order_groups(full, order_by, limit)
    with plan_mode(mode):
        p = eng.compile_plan(t, group_cols=group_cols, aggs=aggs,
                             order_by=order_by, limit=limit,
                             est_groups=est_groups)
        for r in range(repeats):
            got = eng.execute_plan(p, max_groups=len(full) + 1)
            assert got == exp, (r, order_by, limit, _first_diff(got, exp))
        dev = launches(eng, p, "path_plan_topk_device")
        host = launches(eng, p, "path_plan_topk_host")
        os.environ["GG_PLAN_TOPK"] = "host"
        try:
            got = eng.execute_plan(p, max_groups=len(full) + 1)
        finally:
            del os.environ["GG_PLAN_TOPK"]
        assert got == exp, ("host", order_by, limit, _first_diff(got, exp))
        assert launches(eng, p, "path_plan_topk_host") == host + 1
        assert launches(eng, p, "path_plan_topk_device") == dev
    return p, exp, dev, host


def _first_diff(got, exp):
    if len(got) != len(exp):
        return ("length", len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        if g != e:
            return (i, g, e)
    return None


class Tab(dict):
    pass


def make_tab(eng, name, cols, nullmap):
    """a registered table and a memo of its unordered reference results,
    one eval_plan per (group columns, aggregates)"""
    t, data, nulls = register(eng, name, cols, nullmap)
    n = len(cols[0][2])
    memo = {}

    def full(group_cols, aggs):
        k = repr((group_cols, aggs))
        if k not in memo:
            memo[k] = eval_plan(n, data, nulls, [], [], group_cols, aggs)
        return memo[k]
    return Tab(t=t, full=full, n=n)


def _dup(rng, keys, extra):
    """one row per key plus `extra` duplicate rows, shuffled"""
    rows = np.concatenate([keys, rng.choice(keys, extra)])
    return rows[rng.permutation(len(rows))]


# ---- ordering: each kind of order key alone, ASC and DESC ----

@pytest.fixture(scope="module")
def single(eng):
    """~640 groups by one nullable int64 key; m is NULL on 30% of the rows,
    so that many (mostly one-row) groups have a NULL MIN/MAX"""
    rng = np.random.default_rng(5101)
    keys = (rng.permutation(5000)[:640] * 7919 - 10 ** 7).astype(np.int64)
    k = _dup(rng, keys, 40)
    n = len(k)
    cols = [("k", "int64", k),
            ("x", "int64", rng.integers(-1000, 1000, n).astype(np.int64)),
            ("m", "int32", rng.integers(-50, 50, n).astype(np.int32))]
    nullmap = {"k": rng.random(n) < 0.02, "m": rng.random(n) < 0.3}
    return make_tab(eng, "po_single", cols, nullmap)


@pytest.fixture(scope="module")
def carry(eng):
    """test_gpu_plan_carry's many-groups shape: ~500 groups of ~40 rows
    whose SUM(a*b) passes 2^64.  Its sums drift upwards; b is negated for
    the odd keys here, so that they pass -2^64 as well"""
    from test_gpu_plan_carry import _many_groups
    cols, nullmap, _g = _many_groups()
    cols = dict((c, (t, a)) for c, t, a in cols)
    k, b = cols["k"][1], cols["b"][1]
    cols["b"] = ("int64", np.where(k % 2 == 0, b, -b).astype(np.int64))
    return make_tab(eng, "po_carry",
                    [(c, t, a) for c, (t, a) in cols.items()], nullmap)


@pytest.fixture(scope="module")
def pair(eng):
    """~900 groups by a packed pair (nullable int32, nullable int64)"""
    rng = np.random.default_rng(5102)
    code = rng.permutation(40 * 60)[:900]
    code = _dup(rng, code, 50)
    n = len(code)
    cols = [("g0", "int32", (code // 60 - 20).astype(np.int32)),
            ("g1", "int64", (code % 60 * 10 ** 6 - 7).astype(np.int64)),
            ("x", "int64", rng.integers(0, 3, n).astype(np.int64)),
            ("m", "int32", rng.integers(0, 2, n).astype(np.int32))]
    nullmap = {"g0": rng.random(n) < 0.05, "g1": rng.random(n) < 0.05,
               "m": rng.random(n) < 0.3}
    return make_tab(eng, "po_pair", cols, nullmap)


@pytest.fixture(scope="module")
def chars(eng):
    """~700 groups by two nullable char1 columns, bytes up to 255"""
    rng = np.random.default_rng(5103)
    alpha = np.concatenate([np.arange(0, 15), np.arange(241, 256)])
    code = _dup(rng, rng.permutation(900)[:700], 40)
    n = len(code)
    cols = [("c0", "char1", alpha[code // 30].astype(np.uint8)),
            ("c1", "char1", alpha[code % 30].astype(np.uint8)),
            ("x", "int64", rng.integers(-9, 9, n).astype(np.int64))]
    nullmap = {"c0": rng.random(n) < 0.05, "c1": rng.random(n) < 0.05}
    return make_tab(eng, "po_chars", cols, nullmap)


DIRS = ["asc", "desc"]
SUMX = ("sum", [("x", "id")])


@pytest.mark.parametrize("direction", DIRS)
def test_order_by_count(eng, single, direction):
    aggs = ["count", SUMX]
    _p, exp, dev, _h = run_ordered(eng, single, ["k"], aggs,
                                   [("agg", 0, direction)], 10)
    assert dev == 1 and len(exp) == 10
    # counts tie (most groups hold one row): the keys decided
    assert len({g[2][0] for g in exp}) < len(exp)


@pytest.mark.parametrize("direction", DIRS)
def test_order_by_negative_sum(eng, single, direction):
    _p, exp, dev, _h = run_ordered(eng, single, ["k"], ["count", SUMX],
                                   [("agg", 1, direction)], 25)
    assert dev == 1
    assert (exp[0][2][1] < 0) == (direction == "asc")


@pytest.mark.parametrize("direction", DIRS)
def test_order_by_sum_beyond_two_words(eng, carry, direction):
    aggs = [("sum", [("a", "id"), ("b", "id")]), "count"]
    full = carry["full"](["k"], aggs)
    assert max(g[2][0] for g in full) > 1 << 64
    assert min(g[2][0] for g in full) < -(1 << 64)
    _p, exp, dev, _h = run_ordered(eng, carry, ["k"], aggs,
                                   [("agg", 0, direction)], 20)
    assert dev == 1
    assert (exp[0][2][0] > 1 << 64) if direction == "desc" else (
        exp[0][2][0] < -(1 << 64))


@pytest.mark.parametrize("nulls", ["nulls_first", "nulls_last"])
@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("kind", ["min", "max"])
def test_order_by_minmax_with_null_groups(eng, single, kind, direction,
                                          nulls):
    aggs = [(kind, ("m", "id")), "count"]
    full = single["full"](["k"], aggs)
    nnull = sum(g[2][0] is None for g in full)
    assert 50 < nnull < len(full) - 50
    # a limit inside the NULL groups, and one that crosses their edge
    for limit in (10, nnull + 5):
        _p, exp, dev, _h = run_ordered(eng, single, ["k"], aggs,
                                       [("agg", 0, direction, nulls)],
                                       limit)
        assert dev == 1
        assert (exp[0][2][0] is None) == (nulls == "nulls_first")


@pytest.mark.parametrize("direction", DIRS)
def test_order_by_null_placement_default(eng, single, direction):
    """the binding's default: NULLS LAST for ASC, NULLS FIRST for DESC"""
    aggs = [("max", ("m", "id"))]
    _p, exp, dev, _h = run_ordered(eng, single, ["k"], aggs,
                                   [("agg", 0, direction)], 10)
    assert dev == 1 and (exp[0][2][0] is None) == (direction == "desc")


@pytest.mark.parametrize("nulls", ["nulls_first", "nulls_last"])
@pytest.mark.parametrize("direction", DIRS)
def test_order_by_single_key_with_nulls(eng, single, direction, nulls):
    _p, exp, dev, _h = run_ordered(eng, single, ["k"], ["count"],
                                   [("key", 0, direction, nulls)], 10)
    assert dev == 1
    assert (exp[0][0] == NULL_KEY) == (nulls == "nulls_first")
    # and with every group: the NULL key at the end asked for
    _p, exp, dev, host = run_ordered(eng, single, ["k"], ["count"],
                                     [("key", 0, direction, nulls)], 0)
    assert dev == 0 and host == 1
    assert exp[0 if nulls == "nulls_first" else -1][0] == NULL_KEY


@pytest.mark.parametrize("nulls", ["nulls_first", "nulls_last"])
@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("g", [0, 1])
def test_order_by_packed_pair_key(eng, pair, g, direction, nulls):
    p, exp, dev, _h = run_ordered(eng, pair, ["g0", "g1"], ["count", SUMX],
                                  [("key", g, direction, nulls)], 60)
    assert dev == 1 and "path_plan_group_packed" in stats_of(eng, p)
    assert (exp[0][g] == NULL_KEY) == (nulls == "nulls_first")


@pytest.mark.parametrize("nulls", ["nulls_first", "nulls_last"])
@pytest.mark.parametrize("direction", DIRS)
@pytest.mark.parametrize("g", [0, 1])
def test_order_by_char_pair_key(eng, chars, g, direction, nulls):
    p, exp, dev, _h = run_ordered(eng, chars, ["c0", "c1"], ["count", SUMX],
                                  [("key", g, direction, nulls)], 60)
    assert dev == 1 and "path_plan_group_packed" not in stats_of(eng, p)
    assert (exp[0][g] == NULL_KEY) == (nulls == "nulls_first")
    if nulls == "nulls_last":
        # bytes compare as 0..255, not as signed chars
        assert exp[0][g] == (255 if direction == "desc" else 0)


@pytest.mark.parametrize("tab", ["pair", "chars"])
def test_limit_alone_is_key_order(eng, pair, chars, tab):
    """no order entry: the (key0, key1) order, NULL keys first in both"""
    table, gc = (pair, ["g0", "g1"]) if tab == "pair" else (chars,
                                                            ["c0", "c1"])
    _p, exp, dev, _h = run_ordered(eng, table, gc, ["count"], [], 100)
    assert dev == 1 and exp[0][0] == NULL_KEY
    assert [(g[0], g[1]) for g in exp] == sorted((g[0], g[1]) for g in exp)
    assert len({g[0] for g in exp}) > 1      # into the non-NULL key0s


def test_four_entries_tie_break_decides(eng, pair):
    """COUNT, MIN(m), key0 and SUM(x) take a handful of values each, so
    most neighbours tie on all four and (key0, key1) orders them"""
    aggs = ["count", ("min", ("m", "id")), SUMX]
    by = [("agg", 0, "desc"), ("agg", 1, "asc", "nulls_first"),
          ("key", 0, "desc", "nulls_last"), ("agg", 2, "desc")]
    full = pair["full"](["g0", "g1"], aggs)

    def four(g):
        return (g[2][0], g[2][1], g[0], g[2][2])
    assert len({four(g) for g in full}) < len(full) // 2
    for limit in (200, 0):
        _p, exp, dev, _h = run_ordered(eng, pair, ["g0", "g1"], aggs, by,
                                       limit)
        assert dev == (1 if limit else 0)
        ties = sum(four(a) == four(b) for a, b in zip(exp, exp[1:]))
        assert ties > len(exp) // 4


# ---- the device path's boundaries ----

def _count_tab(eng, ng):
    rng = np.random.default_rng(5200 + ng)
    keys = (rng.permutation(4 * ng)[:ng] * 3 - ng).astype(np.int64)
    k = _dup(rng, keys, max(1, ng // 25))
    cols = [("k", "int64", k),
            ("x", "int64", rng.integers(-1000, 1000, len(k)).astype(
                np.int64))]
    return make_tab(eng, f"po_count_{ng}", cols, {})


_COUNT_TABS = {}


@pytest.fixture(scope="module")
def count_tab(eng):
    def get(ng):
        if ng not in _COUNT_TABS:
            _COUNT_TABS[ng] = _count_tab(eng, ng)
        return _COUNT_TABS[ng]
    yield get
    _COUNT_TABS.clear()


# group counts as functions of (limit, tile): limit + 1, the tile size and
# its neighbours, and a count that takes three rounds at the largest limit
# (two tiles' worth of survivors after the first round).  The constants come
# from the library when the test runs, not when it is collected.
NG_OF = {"limit+1": lambda limit, tile: limit + 1,
         "tile-1": lambda limit, tile: tile - 1,
         "tile": lambda limit, tile: tile,
         "tile+1": lambda limit, tile: tile + 1,
         "2*tile+1": lambda limit, tile: 2 * tile + 1}


@pytest.mark.parametrize("groups", list(NG_OF))
@pytest.mark.parametrize("lim", ["1", "10", "max"])
def test_device_topk_boundaries(eng, count_tab, lim, groups):
    max_limit, tile = _consts()
    limit = max_limit if lim == "max" else int(lim)
    ng = NG_OF[groups](limit, tile)
    tab = count_tab(ng)
    p, exp, dev, host = run_ordered(eng, tab, ["k"], [SUMX, "count"],
                                    [("agg", 0, "desc")], limit)
    assert len(exp) == limit
    if ng <= 8:         # limit + 1 = 2 groups: left to the host
        assert (dev, host) == (0, 1)
        return
    assert (dev, host) == (1, 0)
    st = stats_of(eng, p)["plan_topk"]
    # rounds: the survivors of a round are its tiles x limit
    rounds, n = 1, ng
    while n > tile:
        n = -(-n // tile) * limit
        rounds += 1
    assert st["launches"] == rounds and st["rows_in"] == ng
    if (ng, limit) == (2 * tile + 1, max_limit):
        assert rounds >= 3


# ---- what goes to the host path ----

def test_limit_above_device_cap_orders_on_host(eng, count_tab):
    max_limit, tile = _consts()
    _p, exp, dev, host = run_ordered(eng, count_tab(tile + 1), ["k"],
                                     [SUMX, "count"], [("agg", 0, "asc")],
                                     max_limit + 1)
    assert (dev, host) == (0, 1) and len(exp) == max_limit + 1


def test_order_without_limit_returns_every_group(eng, count_tab):
    _max_limit, tile = _consts()
    _p, exp, dev, host = run_ordered(eng, count_tab(tile + 1), ["k"],
                                     [SUMX, "count"], [("agg", 0, "desc")],
                                     0)
    assert (dev, host) == (0, 1) and len(exp) == tile + 1


def test_fewer_groups_than_limit_returns_all_ordered(eng, count_tab):
    max_limit, _tile = _consts()
    _p, exp, dev, host = run_ordered(eng, count_tab(11), ["k"],
                                     [SUMX, "count"], [("agg", 0, "desc")],
                                     max_limit)
    assert (dev, host) == (0, 1) and len(exp) == 11
    _p, exp, dev, host = run_ordered(eng, count_tab(11), ["k"],
                                     [SUMX, "count"], [("agg", 0, "desc")],
                                     11)
    assert (dev, host) == (0, 1) and len(exp) == 11


def test_baked_kernel_under_an_order(eng):
    """4 groups: the second-stage bake keeps its whole group set, and the
    executes it serves come out ordered and limited like the first"""
    rng = np.random.default_rng(5300)
    n = 3000
    cols = [("c0", "char1", rng.choice(np.frombuffer(b"AN", np.uint8), n)),
            ("c1", "char1", rng.choice(np.frombuffer(b"FO", np.uint8), n)),
            ("x", "int64", rng.integers(-50, 100, n).astype(np.int64))]
    tab = make_tab(eng, "po_baked", cols, {})
    for limit in (3, 0):
        p, exp, dev, host = run_ordered(eng, tab, ["c0", "c1"],
                                        [SUMX, "count"],
                                        [("agg", 0, "desc")], limit,
                                        mode="rtc", repeats=3)
        assert (dev, host) == (0, 3) and len(exp) == (limit or 4)
        assert {"path_plan_rtc_baked", "path_plan_rtc_baked_fast"} & set(
            stats_of(eng, p))


def test_plain_aggregate_with_order_yields_its_row(eng, single):
    _p, exp, dev, host = run_ordered(eng, single, [], ["count", SUMX],
                                     [("agg", 1, "desc")], 5)
    assert (dev, host) == (0, 1) and len(exp) == 1


# ---- the growable group table ----

NGROW = 270_000         # distinct keys: more than the fixed 2^18 slots


@pytest.fixture(scope="module")
def big(eng):
    """270,000 groups by one int64 key, 3% duplicate rows.  The reference
    is direct numpy here (exact: the sums stay far inside int64), because
    the evaluator's per-group Python loop would take minutes at this size"""
    rng = np.random.default_rng(5400)
    keys = (rng.permutation(2 * NGROW)[:NGROW] * 5 - NGROW).astype(np.int64)
    k = _dup(rng, keys, 8000)
    x = rng.integers(-10 ** 6, 10 ** 6, len(k)).astype(np.int64)
    t = eng.register_table("po_big", [("k", "int64", k), ("x", "int64", x)],
                           len(k))
    uk, inv = np.unique(k, return_inverse=True)
    sums = np.zeros(len(uk), np.int64)
    np.add.at(sums, inv, x)
    cnts = np.bincount(inv, minlength=len(uk))
    full = [(int(a), 0, [int(s), int(c)])
            for a, s, c in zip(uk, sums, cnts)]
    assert len(full) == NGROW
    return t, full


def _run_big(eng, big, est, executes):
    t, full = big
    by, limit = [("agg", 0, "desc")], 1000
    exp = order_groups(full, by, limit)
    p = eng.compile_plan(t, group_cols=["k"], aggs=[SUMX, "count"],
                         order_by=by, limit=limit, est_groups=est)
    grows = []
    for _ in range(executes):
        assert eng.execute_plan(p) == exp
        grows.append(launches(eng, p, "path_plan_group_grow"))
    assert launches(eng, p, "path_plan_topk_device") == executes
    return grows


def test_good_estimate_needs_no_regrow(eng, big):
    assert _run_big(eng, big, 300_000, 2) == [0, 0]


def test_underestimate_regrows_once_on_first_execute_only(eng, big):
    """est_groups = 1 starts on the fixed 2^18 slots, which 270,000 groups
    fill: the ~8,000 groups that arrive late each probe the whole table
    before the scan is redone on 2^20 slots (the ceiling for these rows).
    The second execute starts on the remembered size.  Measured on one
    MI355X: 0.62 s for this test's two executes, against 0.41 s for the
    well-estimated plan's."""
    assert _run_big(eng, big, 1, 2) == [1, 1]


def test_no_estimate_keeps_the_fixed_cap(eng, big):
    from greengage_amd import EngineError
    t, _full = big
    p = eng.compile_plan(t, group_cols=["k"], aggs=[SUMX, "count"],
                         order_by=[("agg", 0, "desc")], limit=1000)
    with pytest.raises(EngineError, match="group cardinality exceeds"):
        eng.execute_plan(p)
    assert launches(eng, p, "path_plan_group_grow") == 0


# ---- errors ----

def test_compile_errors(eng, single):
    from greengage_amd import engine as ge
    t = single["t"]

    def status(order_by=(), limit=0, est_groups=0, edit=None,
               group_cols=("k",), aggs=("count", SUMX)):
        d = ge.build_plan_desc(t, group_cols=list(group_cols),
                               aggs=list(aggs), order_by=list(order_by),
                               limit=limit, est_groups=est_groups)[0]
        if edit:
            edit(d)
        h = ctypes.c_int32()
        return ge.lib().gg_engine_compile_plan(ctypes.byref(d),
                                               ctypes.byref(h))

    def setf(**kw):
        def edit(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return edit

    def order0(**kw):
        def edit(d):
            for k, v in kw.items():
                setattr(d.order[0], k, v)
        return edit

    ok = [("agg", 0, "desc")]
    assert status(ok, 5, 7) == 0
    assert status(ok, ge.PLAN_MAX_LIMIT + 5) == 0
    # GG_ENOTSUP
    assert status(ok, -1) == ENOTSUP
    assert status(ok, 0, -1) == ENOTSUP
    assert status(ok, edit=setf(norder=ge.PLAN_MAX_ORDER + 1)) == ENOTSUP
    assert status(ok, edit=setf(norder=-1)) == ENOTSUP
    assert status([("agg", 2, "asc")],
                  aggs=["count", SUMX, ("avg", [("x", "id")])]) == ENOTSUP
    # GG_EINVAL
    assert status(ok, edit=order0(what=2)) == EINVAL
    assert status(ok, edit=order0(what=-1)) == EINVAL
    assert status([("key", 1, "asc")]) == EINVAL          # one group column
    assert status([("key", 0, "asc")], group_cols=()) == EINVAL
    assert status([("key", -1, "asc")]) == EINVAL
    assert status([("agg", 2, "asc")]) == EINVAL          # two aggregates
    assert status([("agg", -1, "asc")]) == EINVAL
    ge.lib().gg_engine_last_error.restype = ctypes.c_char_p
    assert b"order entry" in ge.lib().gg_engine_last_error()
    # a plain aggregate takes an order and a limit
    assert status(ok, 3, group_cols=()) == 0
