"""Directed cases for three and four group columns in compiled plans
(engine_abi.h gg_plan_groups): the code e0 || e1 || ... of G packed fields,
e = 0 for NULL, else v - min + 1, field 0 most significant.

Every case is compared bit for bit, and in arena order, with
plan_groupn_ref.eval_plan through its run(): three executes, so a plan with
at most 8 groups runs the baked kernel on executes 2 and 3.  Each runs on the
generated kernels and on the interpreted kernel (GG_PLAN_RTC=0).  The tables
are registered once per module: 19,997 driving rows, build tables of 301 and
257 rows.  Two cases need other sizes: the regrow of the group table shows
only past its 2^19 fixed slots (530,000 groups, checked against numpy), and
the Q3 cross-check runs the SF1 tables of test_gpu_engine.py.
"""
import ctypes
import os

import numpy as np
import pytest

import plan_groupn_ref as ref
from plan_groupn_ref import NULL_KEY, join, plan_mode, register, run, strip

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = "status 1:", "status 5:"
N = 19_997
K = 3                          # width case: every column spans 2^K values
M0, M1, M2 = -7, 1 << 33, 240  # ... from these minima
E31 = (1 << 31) - 2            # [0, E31] takes 31 bits
E30 = (1 << 30) - 2            # [0, E30] takes 30
AGGS = ["count", ("sum", [("v", "id")]), ("min", ("v", "id")),
        ("avg", [("v", "sub100")])]


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


@pytest.fixture(scope="module")
def drive(eng):
    rng = np.random.default_rng(2126)
    # width case: full ranges; rows 0 and 1 hold every maximum and every
    # minimum together, rows 2.. the mixed corners
    w = [rng.integers(m, m + (1 << K), N) for m in (M0, M1, M2)]
    top = [m + (1 << K) - 1 for m in (M0, M1, M2)]
    for r in range(8):
        for g, m in enumerate((M0, M1, M2)):
            w[g][r] = top[g] if (r >> g) & 1 == 0 else m
    # budget edge: 31 + 30 + 1 bits; e1x is e1 with ONE value one larger
    e0 = rng.choice([0, E31], N)
    e1 = rng.choice([0, E30], N)
    e0[:2], e1[:2] = [0, E31], [0, E30]
    e1x = e1.copy()
    e1x[1] = E30 + 1
    cols = [
        ("v", "int64", rng.integers(-1000, 100_000, N).astype(np.int64)),
        ("c1", "char1", rng.integers(65, 70, N).astype(np.uint8)),
        ("i32", "int32", rng.integers(-3, 9, N).astype(np.int32)),
        ("i64", "int64", (rng.integers(0, 11, N) * 1_000_003 - 5_000_000)
         .astype(np.int64)),
        # 60 x 5 x 10 = 3,000 groups
        ("a32", "int32", rng.integers(-60, 0, N).astype(np.int32)),
        ("b5", "int64", (rng.integers(0, 5, N) * 7 - (1 << 40))
         .astype(np.int64)),
        ("c10", "char1", rng.integers(200, 210, N).astype(np.uint8)),
        # 2 x 2 x 2 = 8 groups
        ("s0", "int32", rng.integers(0, 2, N).astype(np.int32)),
        ("s1", "int64", rng.choice([-3, 4], N).astype(np.int64)),
        ("s2", "char1", rng.integers(65, 67, N).astype(np.uint8)),
        ("w0", "int32", w[0].astype(np.int32)),
        ("w1", "int64", w[1].astype(np.int64)),
        ("w2", "char1", w[2].astype(np.uint8)),
        ("e0", "int64", e0.astype(np.int64)),
        ("e1", "int64", e1.astype(np.int64)),
        ("e1x", "int64", e1x.astype(np.int64)),
        ("one", "int32", np.full(N, -5, np.int32)),
        ("fk0", "int64", rng.integers(0, 320, N).astype(np.int64)),
        ("fk1", "int64", ((rng.integers(0, 270, N) - 130) * 1000 + 7)
         .astype(np.int64)),
    ]
    nullmap = {c: rng.random(N) < 0.2 for c in ("c1", "i32", "i64")}
    return register(eng, "gn_drive", cols, nullmap)


@pytest.fixture(scope="module")
def builds(eng):
    """b0: dense keys 1..301 (index map), probed by fk0 in [0, 320): rows
    without a partner.  b1: sparse keys around zero (hash map), probed by fk1,
    of whose 270 values 257 are keys.  Both carry nullable payload columns."""
    rng = np.random.default_rng(2127)
    m0, m1 = 301, 257
    k1 = ((rng.permutation(np.arange(m1)) - m1 // 2) * 1000 + 7)
    b0 = register(eng, "gn_b0", [
        ("bk", "int64", rng.permutation(np.arange(1, m0 + 1)).astype(np.int64)),
        ("nat", "int32", rng.integers(-4, 5, m0).astype(np.int32)),
        ("keep", "int32", rng.integers(0, 10, m0).astype(np.int32))],
        {"nat": rng.random(m0) < 0.15})
    b1 = register(eng, "gn_b1", [
        ("bk", "int64", k1.astype(np.int64)),
        ("year", "int64", (1992 + rng.integers(0, 4, m1)).astype(np.int64)),
        ("keep", "int32", rng.integers(0, 10, m1).astype(np.int32))],
        {"year": rng.random(m1) < 0.15})
    return b0, b1


def stat(eng, p, name):
    return next((s["launches"] for s in eng.stats(p) if s["name"] == name), 0)


def env(name, value):
    """context manager: one environment variable for the executes inside"""
    import contextlib

    @contextlib.contextmanager
    def cm():
        os.environ[name] = value
        try:
            yield
        finally:
            os.environ.pop(name, None)
    return cm()


# ---- codes ----

def test_char1_int32_int64_with_nulls_in_each(eng, mode, drive):
    t, d, nl = drive
    _p, exp, paths = run(eng, mode, t, d, nl, [("v", 0, 90_000)], [],
                         ["c1", "i32", "i64"], AGGS)
    keys = {g[0] for g in exp}
    assert 900 < len(keys) <= 6 * 13 * 12
    # a NULL in each position, beside the same two other values: the three
    # stay distinct groups, and distinct from the all-NULL group
    a, b = 66, 3
    c = int(d["i64"].min())
    assert (NULL_KEY, b, c) in keys and (a, NULL_KEY, c) in keys
    assert (a, b, NULL_KEY) in keys and (NULL_KEY,) * 3 in keys
    assert {"path_plan_group_packed", "path_plan_group_packed_n"} <= paths


def test_four_columns_two_payloads_inner_and_left(eng, mode, drive, builds):
    """group by (c1, b0.nat, s1, b1.year): join 0 INNER on a dense index map,
    join 1 LEFT on a hash map with partnerless rows, whose year then reads as
    NULL beside the rows whose year is NULL by its own flag"""
    t, d, nl = drive
    (t0, d0, n0), (t1, d1, n1) = builds
    joins = [join(t0, d0, n0, "bk", "fk0", preds=[("keep", 1, 10)]),
             join(t1, d1, n1, "bk", "fk1", kind="left",
                  preds=[("keep", 0, 8)])]
    m, ridx = ref.resolve_joins(N, d, nl, [], joins)
    assert 0 < (m & (ridx[1] < 0)).sum() < m.sum() < N
    _p, exp, paths = run(eng, mode, t, d, nl, [], joins,
                         ["c1", (0, "nat"), "s1", (1, "year")], AGGS)
    keys = {g[0] for g in exp}
    assert len(keys) > 300
    assert any(k[1] == NULL_KEY for k in keys)
    assert any(k[3] == NULL_KEY for k in keys)
    assert {"path_plan_join_index_dense", "path_plan_join_index_hash",
            "path_plan_join_left", "path_plan_group_packed_n"} <= paths, paths


def test_eight_groups_bake(eng, mode, drive):
    t, d, nl = drive
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["s0", "s1", "s2"], AGGS)
    assert [g[0] for g in exp] == [(a, b, c) for a in (0, 1) for b in (-3, 4)
                                   for c in (65, 66)]
    assert "path_plan_group_packed_n" in paths, paths
    if mode == "rtc":
        assert any(s.startswith("path_plan_rtc_baked") for s in paths), paths
    else:
        assert "path_plan_interp" in paths, paths


def test_three_thousand_groups_overflow_the_block_cache(eng, mode, drive):
    t, d, nl = drive
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["a32", "b5", "c10"],
                         AGGS)
    assert 2900 < len(exp) <= 3000
    assert "path_plan_group_packed_n" in paths, paths


def test_no_field_carries_into_its_neighbour(eng, mode, drive):
    """every column spans exactly 2^K values, and single rows hold all
    maxima, all minima and each mixed corner: a field one bit too narrow
    would carry into the next"""
    t, d, nl = drive
    tops = []
    for c, m in (("w0", M0), ("w1", M1), ("w2", M2)):
        assert (d[c].min(), d[c].max()) == (m, m + (1 << K) - 1)
        tops.append(m + (1 << K) - 1)
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["w0", "w1", "w2"],
                          AGGS)
    assert len(exp) == 1 << (3 * K)
    assert exp[0][0] == (M0, M1, M2) and exp[-1][0] == tuple(tops)
    # four columns, the single-valued one in the middle (one bit)
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [],
                          ["w2", "one", "w1", "w0"], AGGS)
    assert len(exp) == 1 << (3 * K)
    assert exp[-1][0] == (tops[2], -5, tops[1], tops[0])


def test_budget_edge(eng, mode, drive):
    """31 + 30 + 1 bits are exact; one maximum one larger is 31 + 31 + 1,
    refused with GG_ENOTSUP at every execute, and the engine runs the next
    plan"""
    from greengage_amd import EngineError, plan_group_bits_n
    t, d, nl = drive
    assert plan_group_bits_n([0, 0, -5], [E31, E30, -5]) == (0, (31, 30, 1))
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["e0", "e1", "one"],
                          AGGS)
    assert [g[0] for g in exp] == [(a, b, -5) for a in (0, E31)
                                   for b in (0, E30)]
    with plan_mode(mode):
        p = eng.compile_plan(t, group_cols=["e0", "e1x", "one"], aggs=AGGS)
        for _ in range(2):
            with pytest.raises(EngineError) as ei:
                eng.execute_plan_keys(p, max_groups=16)
            assert ENOTSUP in str(ei.value), ei.value
            assert "31 + 31 + 1 bits" in str(ei.value), ei.value
    assert stat(eng, p, "path_plan_group_packed_n") == 0
    run(eng, mode, t, d, nl, [], [], ["one", "e1", "e0"], AGGS, repeats=1)


# ---- ORDER BY / LIMIT, HAVING, the group table ----

def test_order_by_key2_desc_nulls_first_topk(eng, mode, drive):
    t, d, nl = drive
    cols = ["c1", "i32", "i64"]
    by, limit = [("key", 2, "desc", "nulls_first"), ("agg", 1, "desc")], 12
    full = ref.eval_plan(N, d, nl, [], [], cols, AGGS)
    assert len(full) > max(limit, 8)
    exp = ref.order_groups(full, by, limit)
    assert all(g[0][2] == NULL_KEY for g in exp)
    p, _e, paths = run(eng, mode, t, d, nl, [], [], cols, AGGS, exp=exp,
                       order_by=by, limit=limit)
    assert stat(eng, p, "path_plan_topk_device") == 3, paths
    with env("GG_PLAN_TOPK", "host"):
        p, _e, paths = run(eng, mode, t, d, nl, [], [], cols, AGGS, exp=exp,
                           order_by=by, limit=limit)
    assert stat(eng, p, "path_plan_topk_host") == 3
    assert stat(eng, p, "path_plan_topk_device") == 0
    # ... and ascending on key 1 with NULLS LAST, tie-break on the tuple
    by = [("key", 1, "asc"), ("key", 0, "desc")]
    run(eng, mode, t, d, nl, [], [], cols, AGGS, order_by=by, limit=40,
        exp=ref.order_groups(full, by, 40))


def test_having_device_and_host(eng, mode, drive):
    t, d, nl = drive
    cols = ["a32", "b5", "c10"]
    having = [("cmp", 0, ">=", 9), [("cmp", 1, "<", 300_000),
                                    ("is_null", 2)]]
    full = ref.eval_plan(N, d, nl, [], [], cols, AGGS)
    exp = ref.filter_groups(full, having)
    assert 8 < len(exp) < len(full)
    p, _e, _paths = run(eng, mode, t, d, nl, [], [], cols, AGGS, exp=exp,
                        having=having)
    assert stat(eng, p, "path_plan_having_device") == 3
    with env("GG_PLAN_HAVING", "host"):
        p, _e, _paths = run(eng, mode, t, d, nl, [], [], cols, AGGS, exp=exp,
                            having=having)
    assert stat(eng, p, "path_plan_having_host") == 3
    # HAVING, ORDER BY and LIMIT together, the keys of field 0 descending
    by = [("key", 0, "desc"), ("agg", 0, "desc")]
    run(eng, mode, t, d, nl, [], [], cols, AGGS, having=having, order_by=by,
        limit=9, exp=ref.order_groups(exp, by, 9))


NGROW = 530_000         # distinct groups: more than the fixed 2^19 slots


def test_underestimate_regrows_the_table(eng):
    """est_groups = 1 starts on the fixed 2^19 slots, which 530,000 groups
    fill; the scan is redone once on 2^21 slots and the second execute starts
    there.  A good estimate never regrows, and no estimate keeps the cap.
    The reference is direct numpy: every group is one row."""
    from greengage_amd import EngineError
    rng = np.random.default_rng(5500)
    i = rng.permutation(NGROW)
    a, b, c = i // 1000, i % 1000 - 500, (i * 7) % 3
    x = rng.permutation(NGROW).astype(np.int64) - 1000
    t = eng.register_table("gn_grow", [
        ("a", "int32", a.astype(np.int32)), ("b", "int64", b.astype(np.int64)),
        ("c", "char1", c.astype(np.uint8)), ("x", "int64", x)], NGROW)
    by, limit = [("agg", 0, "desc")], 100
    top = np.argsort(-x, kind="stable")[:limit]
    exp = [((int(a[r]), int(b[r]), int(c[r])), [int(x[r]), 1]) for r in top]
    kw = dict(group_cols=["a", "b", "c"], aggs=[("sum", [("x", "id")]),
                                                "count"],
              order_by=by, limit=limit)
    for est, grows in ((1, [1, 1]), (600_000, [0, 0])):
        p = eng.compile_plan(t, est_groups=est, **kw)
        seen = []
        for _ in range(2):
            assert eng.execute_plan_keys(p) == exp
            seen.append(stat(eng, p, "path_plan_group_grow"))
        assert seen == grows, (est, seen)
    p = eng.compile_plan(t, **kw)
    with pytest.raises(EngineError, match="group cardinality exceeds"):
        eng.execute_plan_keys(p)


# ---- the arena ----

def test_arena_header_and_row_stride(eng, mode, drive):
    t, d, nl = drive
    for cols in (["s0", "s1", "s2"], ["s0", "s1", "s2", "one"]):
        G = len(cols)
        exp = ref.eval_plan(N, d, nl, [], [], cols, AGGS)
        with plan_mode(mode):
            p = eng.compile_plan(t, group_cols=cols, aggs=AGGS)
            raw = eng.execute_raw(p, 1 << 16)
        slots = 5              # count, sum, min, avg = 2
        assert int.from_bytes(raw[0:8], "little") == len(exp) == 8
        assert int.from_bytes(raw[8:12], "little") == slots
        assert int.from_bytes(raw[12:16], "little") == G
        stride = 8 * G + 16 * slots
        assert len(raw) == 16 + len(exp) * stride
        for r, (keys, vals) in enumerate(exp):
            off = 16 + r * stride
            got = tuple(int.from_bytes(raw[off + 8 * g:off + 8 * g + 8],
                                       "little", signed=True)
                        for g in range(G))
            assert got == keys
            assert int.from_bytes(raw[off + 8 * G:off + 8 * G + 16],
                                  "little", signed=True) == vals[0]
        # an arena one byte short is refused, not overrun
        from greengage_amd import EngineError
        with pytest.raises(EngineError, match="arena too small"):
            eng.execute_raw(p, len(raw) - 1)


def _compile_groups(eng, t, cols, gs, aggs=("count", ("sum", [("v", "id")])),
                    **kw):
    """gg_engine_compile_plan_groups itself: gs = None, or (names, srcs,
    ncols) written into the struct as they are"""
    from greengage_amd import engine as ge
    d, kinds = ge.build_plan_desc(t, group_cols=cols, aggs=list(aggs), **kw)
    g = None
    if gs is not None:
        g = ge._PlanGroups()
        for i, (c, s) in enumerate(zip(gs[0], gs[1])):
            g.cols[i] = c.encode() if c is not None else None
            g.src[i] = s
        g.ncols = gs[2]
    h = ctypes.c_int32()
    rc = ge.lib().gg_engine_compile_plan_groups(
        ctypes.byref(d), None, None, ctypes.byref(g) if g else None,
        ctypes.byref(h))
    err = ge.lib().gg_engine_last_error().decode()
    if rc == 0:
        eng._plan_kinds[h.value] = kinds
    return rc, h.value, err


def test_no_further_columns_is_compile_plan(eng, mode, drive):
    t, d, nl = drive
    aggs = ["count", ("sum", [("v", "id")])]
    for cols in (["i32", "i64"], ["s2"]):
        with plan_mode(mode):
            p0 = eng.compile_plan(t, group_cols=cols, aggs=aggs)
            want = [eng.execute_plan(p0) for _ in range(3)]
            paths0 = sorted((s["name"], s["launches"]) for s in eng.stats(p0)
                            if s["name"].startswith("path"))
            for gs in (None, ([], [], 0), (["one"], [0], 0)):
                rc, p, err = _compile_groups(eng, t, cols, gs)
                assert rc == 0, err
                assert [eng.execute_plan(p) for _ in range(3)] == want
                paths = sorted((s["name"], s["launches"])
                               for s in eng.stats(p)
                               if s["name"].startswith("path"))
                assert paths == paths0
                assert not any("packed_n" in n for n, _l in paths)


# ---- errors ----

def test_compile_errors(eng, drive, builds):
    from greengage_amd import EngineError
    t, _d, _nl = drive
    (t0, _d0, _n0), (t1, _d1, _n1) = builds
    two = ["c1", "i32"]

    def status(rc, err, want, text):
        assert f"status {rc}:" == want, (rc, err)
        assert text in err, err

    rc, _p, err = _compile_groups(eng, t, two, (["i64", "s0"], [0, 0], 3))
    status(rc, err, ENOTSUP, "3 further group columns")
    rc, _p, err = _compile_groups(eng, t, two, (["i64"], [0], -1))
    status(rc, err, ENOTSUP, "-1 further group columns")
    for cols in ([], ["c1"]):
        rc, _p, err = _compile_groups(eng, t, cols, (["i64"], [0], 1))
        status(rc, err, EINVAL, "need ngroup == 2")
    rc, _p, err = _compile_groups(eng, t, two, (["nope"], [0], 1))
    status(rc, err, EINVAL, "group column missing")
    rc, _p, err = _compile_groups(eng, t, two, ([None], [0], 1))
    status(rc, err, EINVAL, "group column missing")
    rc, _p, err = _compile_groups(eng, t, two, (["i64", "nat"], [0, 1], 2))
    status(rc, err, EINVAL, "names source 1, the plan has 0 joins")
    jk = dict(table=t0, build_key="bk", probe_key="fk0")
    for kind, text in (("semi", "a SEMI join"), ("anti", "an ANTI join")):
        rc, _p, err = _compile_groups(eng, t, two, (["nat"], [1], 1),
                                      joins=[dict(jk, kind=kind)])
        status(rc, err, EINVAL, text)
    rc, _p, err = _compile_groups(eng, t, two, (["nat"], [2], 1),
                                  joins=[dict(jk, kind="inner")])
    status(rc, err, EINVAL, "names source 2, the plan has 1 joins")
    rc, _p, err = _compile_groups(eng, t, two, (["nat"], [-1], 1),
                                  joins=[dict(jk, kind="inner")])
    status(rc, err, EINVAL, "names source -1")
    # COUNT(DISTINCT) beside further columns; two columns stay refused
    cd = ["count", ("count_distinct", "v")]
    rc, _p, err = _compile_groups(eng, t, two, (["i64"], [0], 1), aggs=cd)
    status(rc, err, ENOTSUP, "COUNT(DISTINCT) with 3 group columns")
    rc, _p, err = _compile_groups(eng, t, two, None, aggs=cd)
    status(rc, err, ENOTSUP, "COUNT(DISTINCT) with two group columns")
    # an order entry may name key G - 1, not key G
    with pytest.raises(EngineError) as ei:
        eng.compile_plan(t, group_cols=two + ["i64"], aggs=["count"],
                         order_by=[("key", 3, "asc")], limit=5)
    assert EINVAL in str(ei.value) and "the plan has 3" in str(ei.value)
    p = eng.compile_plan(t, group_cols=two + ["i64"], aggs=["count"],
                         order_by=[("key", 2, "asc")], limit=5)
    # execute_plan reports two keys: not for this plan
    with pytest.raises(ValueError):
        eng.execute_plan(p)
    with pytest.raises(ValueError):
        eng.compile_plan(t, group_cols=two * 2 + ["i64"], aggs=["count"])
    assert len(eng.execute_plan_keys(p)) == 5


def test_three_columns_need_the_new_entry_point(eng, drive):
    """a third column is what gg_plan_desc alone refuses"""
    from greengage_amd import engine as ge
    t, _d, _nl = drive
    d, _k = ge.build_plan_desc(t, group_cols=["c1", "i32"], aggs=["count"])
    d.ngroup = 3
    h = ctypes.c_int32()
    assert ge.lib().gg_engine_compile_plan(ctypes.byref(d),
                                           ctypes.byref(h)) == 5


# ---- Q3 as a descriptor ----

def test_q3_descriptor_equals_the_named_pipeline(eng):
    """TPC-H Q3 at SF1, grouped by (l_orderkey, o_orderdate, o_shippriority):
    the same 10 rows as GG_PIPE_Q3"""
    from greengage_amd import PGDate
    from greengage_amd.engine import NEG_INF, PIPE_Q3, POS_INF
    li = eng.register_synth("lineitem", seed=42, sf=1)
    od = eng.register_synth("orders", seed=42, sf=1)
    cu = eng.register_synth("customer", seed=42, sf=1)
    cutoff = PGDate("1995-03-15")
    q3 = eng.compile(PIPE_Q3, lineitem=li, orders=od, customer=cu,
                     cutoff_date=cutoff, mktsegment=2, limit_k=10)
    named, _hdr = eng.execute_q3(q3)
    assert len(named) == 10
    p = eng.compile_plan(
        li, preds=[("shipdate", cutoff + 1, POS_INF)],
        joins=[{"table": od, "build_key": "orderkey", "probe_key": "orderkey",
                "kind": "inner", "preds": [("orderdate", NEG_INF, cutoff)]},
               {"table": cu, "build_key": "custkey", "probe_key": "custkey",
                "kind": "semi", "probe_src": 1, "preds": [("mktseg", 2, 3)]}],
        group_cols=["orderkey", (0, "orderdate"), (0, "shippriority")],
        aggs=[("sum", [("price", "id"), ("disc", "sub100")])],
        order_by=[("agg", 0, "desc"), ("key", 1, "asc")], limit=10,
        est_groups=eng.table_nrows(od))
    for _ in range(2):
        got = eng.execute_plan_keys(p)
        assert [(k[0], v[0], k[1], k[2]) for k, v in got] == \
            [(r["orderkey"], r["revenue4"], r["orderdate"], r["shippriority"])
             for r in named]
    assert stat(eng, p, "path_plan_group_packed_n") == 2
    assert stat(eng, p, "path_plan_topk_device") == 2
