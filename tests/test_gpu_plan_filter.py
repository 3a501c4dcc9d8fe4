"""Per-aggregate FILTER predicates of compiled plans (engine_abi.h
gg_plan_filter), directed cases.

Every case runs on the generated kernels and, under plan_mode("interp"),
on the interpreted kernel, three executes each (the baked kernel takes
over from the second where one is made), and must equal
plan_filter_ref.eval_plan bit for bit.

Sizes are the smallest that reach each accumulator destination, as in
test_gpu_plan_carry.py: no group column at n in {1, 63, 64, 65, 300}
(registers and the wave flush, with a wave in which no lane passes the
filter), 5000 rows in 2x2 char1 groups (LDS cache, then the baked
tables), 20000 rows in 500 int64 groups (global-table fallback).  The
interpreted kernel's 4-row main loop only engages above ~2.1 M rows
(4 x 2048 x 256) and a filter lives wholly in the row body, which both
loops share, so no case needs that size.
"""
import ctypes

import numpy as np
import pytest

from plan_filter_ref import NEG_INF, POS_INF, join, register, run

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = 1, 5
TINY = [1, 63, 64, 65, 300]


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


def flt(agg, preds):
    return ("filter", agg, preds)


def _check_paths(paths, mode, baked=None):
    if mode == "interp":
        assert "path_plan_interp" in paths
        return
    assert "path_plan_rtc" in paths
    if baked:
        assert baked in paths, paths


def _cols(rng, n, signed=True):
    """qty 1..50, disc 0..10, price non-negative unless `signed`"""
    return [("qty", "int32", rng.integers(1, 51, n).astype(np.int32)),
            ("disc", "int64", rng.integers(0, 11, n).astype(np.int64)),
            ("price", "int64",
             rng.integers(-1000 if signed else 0, 100000,
                          n).astype(np.int64)),
            ("day", "int32", rng.integers(8000, 8100, n).astype(np.int32))]


# every aggregate kind under a filter beside its unfiltered twin; `disc`
# is a factor and a filter column at once
F_DISC = [("disc", 3, 8)]
TWINS = [flt("count", F_DISC), "count",
         flt(("sum", [("price", "id"), ("disc", "sub100")]), F_DISC),
         ("sum", [("price", "id"), ("disc", "sub100")]),
         flt(("count", "price"), F_DISC), ("count", "price")]
TWINS_MM = [flt(("min", ("price", "id")), F_DISC), ("min", ("price", "id")),
            flt(("max", ("disc", "add100")), F_DISC),
            flt(("avg", [("price", "id")]), F_DISC),
            ("avg", [("price", "id")])]


@pytest.mark.parametrize("n", TINY)
@pytest.mark.parametrize("aggs", [TWINS, TWINS_MM], ids=["sum", "minmax"])
def test_no_group_registers_and_wave_flush(eng, mode, n, aggs):
    rng = np.random.default_rng(300 + n)
    cols = _cols(rng, n)
    if n >= 65:
        # rows 0..63 are one wave: none of its lanes passes the filter
        cols[1][2][:64] = 9
    nullmap = {"price": rng.random(n) < 0.2} if n > 1 else {}
    t, data, nulls = register(eng, f"pf_tiny_{n}_{len(aggs)}_{mode}", cols,
                              nullmap)
    _p, exp, paths = run(eng, mode, t, data, nulls, [], [], [], aggs)
    assert len(exp) == 1
    _check_paths(paths, mode)


def _char_case(rng, n, signed):
    cols = _cols(rng, n, signed)
    cols += [("g0", "char1", rng.choice(np.frombuffer(b"AN", np.uint8), n)),
             ("g1", "char1", rng.choice(np.frombuffer(b"FO", np.uint8), n))]
    return cols


@pytest.mark.parametrize("signed", [False, True], ids=["fast", "2word"])
def test_lds_cache_then_baked(eng, mode, signed):
    """non-negative factors keep the fast-tier proof: a filter only
    removes inputs, so the whole-column bound still holds"""
    rng = np.random.default_rng(41)
    cols = _char_case(rng, 5000, signed)
    t, data, nulls = register(eng, f"pf_char_{signed}_{mode}", cols, None)
    _p, exp, paths = run(eng, mode, t, data, nulls, [("day", 8000, 8090)],
                         [], ["g0", "g1"], TWINS + TWINS_MM[:1])
    assert len(exp) == 4
    _check_paths(paths, mode, "path_plan_rtc_baked" if signed
                 else "path_plan_rtc_baked_fast")
    if mode == "rtc":
        assert ("path_plan_rtc_baked_fast" in paths) == (not signed)


def test_global_table_fallback(eng, mode):
    rng = np.random.default_rng(42)
    n = 20000
    cols = _cols(rng, n)
    cols.append(("k", "int64",
                 (rng.integers(0, 500, n) * 7919 - 100000).astype(np.int64)))
    t, data, nulls = register(eng, f"pf_many_{mode}", cols,
                              {"price": rng.random(n) < 0.1})
    _p, exp, paths = run(eng, mode, t, data, nulls, [], [], ["k"],
                         TWINS + TWINS_MM[:1])
    assert len(exp) > 400
    _check_paths(paths, mode)


def test_shared_and_overlapping_filters(eng, mode):
    """two aggregates share one filter; two filters overlap in a column"""
    rng = np.random.default_rng(43)
    cols = _char_case(rng, 5000, False)
    f0 = [("disc", 2, 9), ("qty", NEG_INF, 25)]
    f1 = [("qty", 10, POS_INF), ("day", 8010, 8050)]
    aggs = [flt(("sum", [("price", "id")]), f0), flt("count", f0),
            flt(("sum", [("price", "id")]), f1), flt(("count", "qty"), f1),
            ("sum", [("price", "id")])]
    t, data, nulls = register(eng, f"pf_share_{mode}", cols, None)
    _p, _exp, paths = run(eng, mode, t, data, nulls, [], [], ["g0", "g1"],
                          aggs)
    _check_paths(paths, mode, "path_plan_rtc_baked_fast")


def test_nullable_filter_column(eng, mode):
    """group 'Z' has a NULL filter column on every row: it is present and
    reports COUNT 0 / SUM 0 / MIN None / AVG N = 0"""
    rng = np.random.default_rng(44)
    n = 5000
    cols = _cols(rng, n)
    g = rng.choice(np.frombuffer(b"ANZ", np.uint8), n)
    cols.append(("g", "char1", g))
    dn = (rng.random(n) < 0.15) | (g == ord("Z"))
    t, data, nulls = register(eng, f"pf_null_{mode}", cols,
                              {"disc": dn, "price": rng.random(n) < 0.1})
    f = [("disc", NEG_INF, POS_INF)]            # true iff disc is not NULL
    aggs = [flt("count", f), flt(("sum", [("price", "id")]), f),
            flt(("min", ("price", "id")), f),
            flt(("avg", [("qty", "id")]), f), "count"]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], [], ["g"], aggs)
    z = [v for k0, _k1, v in exp if k0 == ord("Z")]
    assert len(exp) == 3 and z and z[0][:4] == [0, 0, None, (0, 0)]
    assert z[0][4] > 0
    _check_paths(paths, mode, "path_plan_rtc_baked")


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_no_row_and_every_row(eng, mode, grouped):
    rng = np.random.default_rng(45)
    n = 5000 if grouped else 300
    cols = _char_case(rng, n, False)
    v = int(cols[0][2][0])
    none = [("qty", 1000, POS_INF)]             # one-sided, nothing passes
    every = [("qty", NEG_INF, 51), ("disc", 0, POS_INF)]
    eq = [("qty", v, v + 1)]                    # equality
    base = ("sum", [("price", "id"), ("qty", "id")])
    aggs = [flt(base, none), flt(base, every), base, flt("count", eq),
            flt(("max", ("price", "id")), none),
            flt(("max", ("price", "id")), every)]
    t, data, nulls = register(eng, f"pf_edge_{grouped}_{mode}", cols, None)
    _p, exp, paths = run(eng, mode, t, data, nulls, [], [],
                         ["g0", "g1"] if grouped else [], aggs)
    for _k0, _k1, vals in exp:
        assert vals[0] == 0 and vals[1] == vals[2] and vals[4] is None
        assert vals[5] is not None
    assert sum(vals[3] for _k0, _k1, vals in exp) == \
        int(np.count_nonzero(cols[0][2] == v))
    _check_paths(paths, mode)


def test_helper_counts(eng, mode):
    from greengage_amd import EngineError
    rng = np.random.default_rng(46)
    cols = _cols(rng, 300)
    t, data, nulls = register(eng, f"pf_help_{mode}", cols,
                              {"price": rng.random(300) < 0.3})
    f = [("disc", 2, 7)]
    # min + max of one column under one filter share a count, the
    # unfiltered avg of it needs its own: 3 value slots + 1 + 1
    aggs = [flt(("min", ("price", "id")), f), flt(("max", ("price", "id")), f),
            ("avg", [("price", "id")])]
    run(eng, mode, t, data, nulls, [], [], [], aggs)
    # four MIN/MAX over four filters: exactly 8 slots
    four = [flt(("min" if k % 2 else "max", ("price", "id")),
                [("disc", k, k + 5)]) for k in range(4)]
    run(eng, mode, t, data, nulls, [], [], [], four)
    with pytest.raises(EngineError, match="status 5:"):
        eng.compile_plan(t, aggs=four + ["count"])
    # the same four under ONE filter share their count: room for more
    one = [flt(a[1], f) for a in four]
    run(eng, mode, t, data, nulls, [], [], [], one + ["count", "count"])


def _orders(eng, name, rng, m, dense, nullmap=None, extra=()):
    keys = rng.permutation(np.arange(1, m + 1)).astype(np.int64)
    if not dense:
        keys = (keys - m // 2) * 1000 + 7
    cols = [("okey", "int64", keys),
            ("odate", "int32", rng.integers(8000, 8400, m).astype(np.int32)),
            ("prio", "char1", rng.integers(0, 5, m).astype(np.uint8))]
    cols += list(extra)
    return (keys,) + register(eng, name, cols, nullmap)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hash"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_payload_filter(eng, mode, dense, grouped):
    """the pivot: SUMs of one expression filtered on ranges of the joined
    row's date, one filter mixing a driving and a payload column, NULL
    flags on the payload column"""
    rng = np.random.default_rng(47)
    m, n = 400, 5000
    keys, ot, od, on = _orders(eng, f"pf_o_{dense}_{grouped}_{mode}", rng, m,
                               dense, {"odate": rng.random(m) < 0.1})
    cols = _char_case(rng, n, False)
    cols.append(("fk", "int64", rng.choice(np.concatenate([keys, [0, -5]]),
                                           n)))
    t, data, nulls = register(eng, f"pf_l_{dense}_{grouped}_{mode}", cols,
                              None)
    rev = ("sum", [("price", "id"), ("disc", "sub100")])
    aggs = [flt(rev, [((0, "odate"), 8000 + 100 * y, 8100 + 100 * y)])
            for y in range(2)]
    aggs += [flt(rev, [((0, "odate"), 8200, POS_INF), ("qty", 1, 25)]), rev,
             flt("count", [((0, "prio"), 1, 3)])]
    joins = [join(ot, od, on, "okey", "fk")]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins,
                         ["g0", "g1"] if grouped else [], aggs)
    _check_paths(paths, mode,
                 "path_plan_rtc_baked_fast" if grouped else None)
    assert ("path_plan_join_index_dense" if dense
            else "path_plan_join_index_hash") in paths
    for _k0, _k1, vals in exp:
        assert 0 < sum(vals[:3]) < vals[3]      # NULL dates pass no range


def test_chained_payload_filter(eng, mode):
    """lineitem -> orders -> customer: filters on the second join's
    payload, and on both joins' at once"""
    rng = np.random.default_rng(48)
    mc, mo, n = 40, 300, 5000
    ckeys = rng.permutation(np.arange(1, mc + 1)).astype(np.int64)
    ct, cd, cn = register(eng, f"pf_c_{mode}", [
        ("ckey", "int64", ckeys),
        ("seg", "char1", rng.integers(0, 5, mc).astype(np.uint8)),
        ("bal", "int64", rng.integers(-999, 9999, mc).astype(np.int64))],
        {"bal": rng.random(mc) < 0.2})
    okeys, ot, od, on = _orders(
        eng, f"pf_co_{mode}", rng, mo, True, None,
        [("ckey", "int64", rng.choice(np.concatenate([ckeys, [77]]), mo))])
    cols = _cols(rng, n, False)
    cols.append(("fk", "int64", rng.choice(okeys, n)))
    t, data, nulls = register(eng, f"pf_cl_{mode}", cols, None)
    joins = [join(ot, od, on, "okey", "fk"),
             join(ct, cd, cn, "ckey", "ckey", probe_src=1)]
    aggs = [flt("count", [((1, "seg"), 2, 3)]),
            flt(("sum", [("price", "id")]), [((1, "bal"), 0, POS_INF)]),
            flt(("min", ((1, "bal"), "id")),
                [((0, "odate"), 8100, 8300), ((1, "seg"), 0, 4)]),
            "count"]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins,
                         [(1, "seg")], aggs)
    assert len(exp) == 5
    _check_paths(paths, mode, "path_plan_rtc_baked_fast")


def test_packed_group_pair(eng, mode):
    """(int32, int64) group columns: the packed-code kernels, filtered"""
    rng = np.random.default_rng(49)
    n = 5000
    cols = _cols(rng, n, False)
    cols += [("ga", "int32", rng.integers(-2, 1, n).astype(np.int32)),
             ("gb", "int64", (rng.integers(0, 2, n) * 10 ** 12).astype(
                 np.int64))]
    t, data, nulls = register(eng, f"pf_gp_{mode}", cols,
                              {"gb": rng.random(n) < 0.1})
    _p, exp, paths = run(eng, mode, t, data, nulls, [], [], ["ga", "gb"],
                         TWINS + TWINS_MM[:1])
    assert len(exp) == 9
    assert "path_plan_group_packed" in paths
    _check_paths(paths, mode)


def test_contract_errors(eng):
    from greengage_amd import engine as ge
    rng = np.random.default_rng(50)
    cols = _cols(rng, 100)
    t, data, nulls = register(eng, "pf_err_l", cols, None)
    bt, bd, bn = register(eng, "pf_err_b", [
        ("k", "int64", np.arange(1, 11, dtype=np.int64)),
        ("w", "int32", np.arange(10, dtype=np.int32))], None)
    good = [flt("count", [("disc", 0, 5)]), "count"]
    semi = [{"table": bt, "build_key": "k", "probe_key": "qty",
             "kind": "semi"}]

    def status(d):
        h = ctypes.c_int32()
        return ge.lib().gg_engine_compile_plan(ctypes.byref(d),
                                               ctypes.byref(h))

    def desc(aggs=good, joins=()):
        return ge.build_plan_desc(t, joins=joins, aggs=aggs)[0]

    d = desc()
    d.aggs[1].filter = 2                        # filter outside [0, nfilters]
    assert status(d) == EINVAL
    d = desc()
    d.aggs[1].filter = -1
    assert status(d) == EINVAL
    d = desc()
    d.nfilters = ge.PLAN_MAX_FILTERS + 1
    assert status(d) == ENOTSUP
    d = desc()
    d.nfilters = -1
    assert status(d) == ENOTSUP
    d = desc()
    d.filters[0].npreds = ge.PLAN_MAX_FILTER_PREDS + 1
    assert status(d) == ENOTSUP
    d = desc()
    d.filters[0].npreds = 0                     # referenced, but empty
    assert status(d) == EINVAL
    d = desc(aggs=[flt("count", [("nosuch", 0, 5)])])
    assert status(d) == EINVAL                  # missing column
    d = desc(aggs=[flt("count", [((0, "w"), 0, 5)])], joins=semi)
    assert status(d) == EINVAL                  # source names a SEMI join
    d = desc(aggs=[flt("count", [((1, "w"), 0, 5)])], joins=semi)
    assert status(d) == EINVAL                  # source names join >= njoins
    # an unreferenced filter is validated the same way ...
    d = desc()
    d.nfilters = 2
    d.filters[1].npreds = 1
    d.filters[1].preds[0].col = b"nosuch"
    assert status(d) == EINVAL
    # ... and otherwise ignored: even an empty one compiles
    d = desc()
    d.nfilters = 2
    assert status(d) == 0
    # the engine stays usable
    for mode in ("rtc", "interp"):
        run(eng, mode, t, data, nulls, [], [], [], good)
