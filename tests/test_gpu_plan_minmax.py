"""Directed cases for MIN / MAX / AVG in compiled plan descriptors.

Every case runs twice: on the default path (hipRTC-generated generic
and baked kernels) and with GG_PLAN_RTC=0 (the interpreted kernel of
plan.hip).  The reference is exact evaluation in plan_minmax_ref; all
comparisons are bit-exact.  The cases aim at where an order-encoded
"unsigned max with identity 0" design goes wrong: the identity itself
(all-negative data, empty input, all-NULL groups), the extreme values
whose encoding IS the identity (INT64_MIN under MAX, INT64_MAX under
MIN), encoding after the 100±col modifier, every accumulator tier
(registers, block LDS cache, global-table overflow, baked 1-word and
2-word tables) and the 4-way strided row loop.
"""
import numpy as np
import pytest

import pyoracle
from plan_minmax_ref import NEG_INF, eval_plan, register, run

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1


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


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_global_group_tiny_all_negative(eng, mode, n):
    rng = np.random.default_rng(n)
    v = rng.integers(-5000, -1, n).astype(np.int64)
    t, data, nulls = register(eng, f"mm_tiny_{mode}_{n}",
                              [("v", "int64", v)])
    aggs = [("max", ("v", "id")), ("min", ("v", "id")),
            ("avg", [("v", "id")]), "count"]
    _p, exp = run(eng, mode, t, data, nulls, [], [], aggs)
    assert exp[0][2][0] < 0 and exp[0][2][1] == int(v.min())


def test_empty_input(eng, mode):
    rng = np.random.default_rng(2)
    n = 1000
    k = rng.integers(0, 5, n).astype(np.int64)
    v = rng.integers(-100, 100, n).astype(np.int64)
    t, data, nulls = register(eng, f"mm_empty_{mode}",
                              [("k", "int64", k), ("v", "int64", v)])
    aggs = [("min", ("v", "id")), ("max", ("v", "id")),
            ("avg", [("v", "id")]), "count"]
    preds = [("v", 1000, 1001)]       # selects nothing
    _p, exp = run(eng, mode, t, data, nulls, preds, [], aggs)
    assert exp == [(0, 0, [None, None, (0, 0), 0])]
    _p, exp = run(eng, mode, t, data, nulls, preds, ["k"], aggs)
    assert exp == []


def test_all_null_inputs_in_live_group(eng, mode):
    rng = np.random.default_rng(3)
    n = 5000
    k = rng.integers(0, 6, n).astype(np.int64)
    v = rng.integers(-100, 100, n).astype(np.int64)
    vnull = (rng.random(n) < 0.2) | (k == 4)    # group 4: all NULL
    t, data, nulls = register(eng, f"mm_allnull_{mode}",
                              [("k", "int64", k), ("v", "int64", v)],
                              {"v": vnull})
    aggs = ["count", ("min", ("v", "id")), ("max", ("v", "id")),
            ("avg", [("v", "id")])]
    # twice: the repeat runs the baked kernel on the default path
    _p, exp = run(eng, mode, t, data, nulls, [], ["k"], aggs, repeats=2)
    g4 = [g for g in exp if g[0] == 4]
    assert len(g4) == 1 and g4[0][2][0] > 0
    assert g4[0][2][1:] == [None, None, (0, 0)]


def test_extremes(eng, mode):
    """INT64_MAX under MIN and INT64_MIN under MAX encode to the
    accumulator's identity 0: only the non-NULL count tells them from
    'no input'."""
    rng = np.random.default_rng(4)
    n = 4000
    k = rng.integers(0, 4, n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    vnull = np.zeros(n, bool)
    # group 0: only non-NULL value is INT64_MAX; group 1: INT64_MIN;
    # groups 2, 3: ordinary data holding both extremes
    for g, x in ((0, I64_MAX), (1, I64_MIN)):
        rows = np.nonzero(k == g)[0]
        vnull[rows] = True
        vnull[rows[7]] = False
        v[rows[7]] = x
    r2 = np.nonzero(k == 2)[0]
    v[r2[0]], v[r2[1]] = I64_MIN, I64_MAX
    t, data, nulls = register(eng, f"mm_ext_{mode}",
                              [("k", "int64", k), ("v", "int64", v)],
                              {"v": vnull})
    aggs = [("min", ("v", "id")), ("max", ("v", "id")), ("count", "v")]
    _p, exp = run(eng, mode, t, data, nulls, [], ["k"], aggs, repeats=2)
    assert exp[0][2] == [I64_MAX, I64_MAX, 1]
    assert exp[1][2] == [I64_MIN, I64_MIN, 1]
    assert exp[2][2][:2] == [I64_MIN, I64_MAX]
    # and as a global group (register accumulators + wave reduction)
    run(eng, mode, t, data, nulls, [("k", 0, 1)], [], aggs)
    run(eng, mode, t, data, nulls, [("k", 1, 2)], [], aggs)


def test_widths_and_modifiers(eng, mode):
    rng = np.random.default_rng(5)
    n = 3000
    k = rng.integers(0, 3, n).astype(np.int64)
    i32 = rng.integers(-50000, -10, n).astype(np.int32)
    c1 = rng.integers(128, 256, n).astype(np.uint8)
    dec = rng.integers(-120, 120, n).astype(np.int64)
    t, data, nulls = register(
        eng, f"mm_width_{mode}",
        [("k", "int64", k), ("i32", "int32", i32), ("c1", "char1", c1),
         ("dec", "dec64", dec)],
        {"dec": rng.random(n) < 0.1})
    for aggs in (
            [("min", ("i32", "id")), ("max", ("i32", "id")),
             ("min", ("c1", "id")), ("max", ("c1", "id"))],
            [("min", ("i32", "sub100")), ("max", ("i32", "add100")),
             ("min", ("dec", "sub100")), ("max", ("dec", "sub100"))],
            [("max", ("c1", "sub100")), ("min", ("c1", "add100")),
             ("min", ("dec", "add100")), ("avg", [("dec", "sub100")])]):
        run(eng, mode, t, data, nulls, [], ["k"], aggs, repeats=2)
        run(eng, mode, t, data, nulls, [], [], aggs)


def test_lds_cache_overflow(eng, mode):
    """~500 groups: more than the 32-slot block cache holds, so rows
    also take the global-table transition."""
    rng = np.random.default_rng(6)
    n = 20000
    k = (rng.integers(0, 500, n) * 7919 - 100000).astype(np.int64)
    v = rng.integers(-100000, 100000, n).astype(np.int64)
    w = rng.integers(-120, 120, n).astype(np.int64)
    t, data, nulls = register(
        eng, f"mm_ovf_{mode}",
        [("k", "int64", k), ("v", "int64", v), ("w", "dec64", w)],
        {"v": rng.random(n) < 0.15})
    aggs = [("min", ("v", "id")), ("max", ("v", "id")),
            ("avg", [("v", "id"), ("w", "sub100")]),
            ("sum", [("w", "id")])]
    _p, exp = run(eng, mode, t, data, nulls, [], ["k"], aggs)
    assert len(exp) > 400


def _baked_table(eng, name, rng, n):
    g0 = rng.choice(np.frombuffer(b"AN", np.uint8), n)
    g1 = rng.choice(np.frombuffer(b"FO", np.uint8), n)
    q = rng.integers(1, 51, n).astype(np.int64)
    d = rng.integers(0, 11, n).astype(np.int64)
    neg = rng.integers(-9000, 9000, n).astype(np.int64)
    return register(
        eng, name,
        [("g0", "char1", g0), ("g1", "char1", g1), ("q", "dec64", q),
         ("d", "dec64", d), ("neg", "int64", neg)],
        {"neg": rng.random(n) < 0.1, "q": rng.random(n) < 0.05})


def test_baked_fast_tier(eng, mode):
    """SUM/AVG inputs small and non-negative: the 1-word fire-and-
    forget tier is provable; MIN/MAX run over a column with negatives
    (their words stay out of the additive bound)."""
    t, data, nulls = _baked_table(eng, f"mm_bakef_{mode}",
                                  np.random.default_rng(7), 50000)
    aggs = [("min", ("neg", "id")), ("max", ("neg", "id")),
            ("avg", [("q", "id"), ("d", "sub100")]),
            ("sum", [("q", "id")])]
    p, exp = run(eng, mode, t, data, nulls, [], ["g0", "g1"], aggs,
                 repeats=4)
    paths = {s["name"] for s in eng.stats(p)}
    assert paths & {"path_plan_rtc_baked_fast",
                    "path_plan_interp"}  # interp-only boxes: no bake

    # AVG finalisation: numeric_avg restated by the oracle
    from greengage_amd import Engine
    for _k0, _k1, vals in exp:
        s, c = vals[2]
        if c:
            assert Engine.avg_str(s, 2, c) == pyoracle.avg_str(s, 2, c)


def test_baked_two_word_tier(eng, mode):
    """A SUM over a column with negatives defeats the overflow-budget
    proof: 2-word accumulators with carry."""
    t, data, nulls = _baked_table(eng, f"mm_bake2_{mode}",
                                  np.random.default_rng(8), 50000)
    aggs = [("min", ("neg", "sub100")), ("max", ("q", "id")),
            ("avg", [("neg", "id")]), ("sum", [("neg", "id"),
                                               ("q", "id")])]
    p, _exp = run(eng, mode, t, data, nulls, [], ["g0", "g1"], aggs,
                  repeats=4)
    paths = {s["name"] for s in eng.stats(p)}
    assert paths & {"path_plan_rtc_baked", "path_plan_interp"}
    assert "path_plan_rtc_baked_fast" not in paths


_BIG = {}


def _big(eng):
    """One table for the 4-way strided loop, shared by both modes: the
    interpreted kernel enters that loop only above 4 x 2048 x 256
    rows."""
    if not _BIG:
        rng = np.random.default_rng(9)
        n = 4 * 2048 * 256 + 1000
        k = rng.integers(0, 40, n).astype(np.int64)
        v = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
        f = rng.integers(0, 100, n).astype(np.int32)
        t, data, nulls = register(
            eng, "mm_big",
            [("k", "int64", k), ("v", "int64", v), ("f", "int32", f)],
            {"v": rng.random(n) < 0.1})
        aggs = [("min", ("v", "id")), ("max", ("v", "id")),
                ("avg", [("v", "id")]), "count"]
        preds = [("f", 10, 95)]
        _BIG.update(
            t=t, data=data, nulls=nulls, aggs=aggs, preds=preds,
            exp0=eval_plan(n, data, nulls, preds, [], [], aggs),
            exp1=eval_plan(n, data, nulls, preds, [], ["k"], aggs))
    return _BIG


def test_four_way_loop_global_group(eng, mode):
    b = _big(eng)
    run(eng, mode, b["t"], b["data"], b["nulls"], b["preds"], [],
        b["aggs"], exp=b["exp0"])


def test_four_way_loop_grouped(eng, mode):
    b = _big(eng)
    _p, exp = run(eng, mode, b["t"], b["data"], b["nulls"], b["preds"],
                  ["k"], b["aggs"], exp=b["exp1"])
    assert len(exp) == 40


def test_limits(eng, mode):
    from greengage_amd.engine import EngineError
    rng = np.random.default_rng(10)
    n = 2000
    cols = [(c, "int64", rng.integers(-500, 500, n).astype(np.int64))
            for c in ("a", "b", "c", "d")]
    t, data, nulls = register(eng, f"mm_lim_{mode}", cols,
                              {"b": rng.random(n) < 0.3})
    with pytest.raises(EngineError, match="status 5"):   # GG_ENOTSUP
        eng.compile_plan(t, aggs=[("min", [("a", "id"), ("b", "id")])])
    # 4 aggregates always fit the accumulator budget, whatever kinds
    for aggs in (
            [("avg", [("a", "id")]), ("avg", [("b", "id")]),
             ("avg", [("c", "id"), ("a", "id")]), ("avg", [("d", "id")])],
            [("min", ("a", "id")), ("max", ("b", "id")),
             ("avg", [("c", "id")]), ("min", ("d", "sub100"))]):
        run(eng, mode, t, data, nulls, [("a", NEG_INF, 400)], [], aggs)
    # past the budget: 5 AVGs over distinct columns need 10 slots
    with pytest.raises(EngineError, match="status 5"):
        eng.compile_plan(t, aggs=[
            ("avg", [("a", "id")]), ("avg", [("b", "id")]),
            ("avg", [("c", "id")]), ("avg", [("d", "id")]),
            ("avg", [("a", "id"), ("b", "id")])])
