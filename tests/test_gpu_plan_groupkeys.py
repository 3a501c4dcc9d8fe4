"""Directed cases for two-column group keys of any type and source in
compiled plans: the packed group code of engine_abi.h
(gg_plan_desc.group_cols), code = (e0 << b1) | e1 with e = 0 for NULL,
else v - min + 1.

Every case is compared bit for bit with plan_payload_ref.eval_plan
through its run(): three executes, so a plan with at most 8 groups runs
the baked kernel on executes 2 and 3.  Each runs on the generated
kernels and on the interpreted kernel (GG_PLAN_RTC=0).  The tables are
registered once per module: 19,997 driving rows, build tables of 301
and 257 rows.
"""
import numpy as np
import pytest

from plan_payload_ref import NULL_KEY, join, plan_mode, register, run

pytestmark = pytest.mark.gpu

ENOTSUP = "status 5:"
N = 19_997
K = 4                          # width case: both columns span 2^K values
M0, M1 = -7, 1 << 33           # ... from these minima
EDGE = (1 << 31) - 2           # [0, EDGE] takes 31 bits
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
    rng = np.random.default_rng(2026)
    # width case: full range, and the two maxima (and minima) in one row
    w0 = rng.integers(M0, M0 + (1 << K), N)
    w1 = rng.integers(M1, M1 + (1 << K), N)
    w0[:4] = [M0 + (1 << K) - 1, M0, M0 + (1 << K) - 1, M0]
    w1[:4] = [M1 + (1 << K) - 1, M1, M1, M1 + (1 << K) - 1]
    # wide values, narrow range: 1,500 pairs drawn from 1000 x 2000
    pool0 = -(1 << 45) + rng.integers(0, 1000, 1500)
    pool1 = (1 << 50) + rng.integers(0, 2000, 1500)
    pool0[:2] = [-(1 << 45), -(1 << 45) + 999]
    pool1[:2] = [(1 << 50) + 1999, 1 << 50]
    pick = rng.integers(0, 1500, N)
    pick[:1500] = np.arange(1500)
    # budget edge: e1x is e1 with ONE value one larger
    e0 = rng.choice([0, EDGE], N)
    e1 = rng.choice([0, EDGE], N)
    e0[:2] = e1[:2] = [0, EDGE]
    e1x = e1.copy()
    e1x[1] = EDGE + 1
    cols = [
        ("v", "int64", rng.integers(-1000, 100_000, N).astype(np.int64)),
        # ~3,000 pairs of negative values; (a, b) has no (b, a) for a < -50
        ("a32", "int32", rng.integers(-60, 0, N).astype(np.int32)),
        ("b64", "int64", rng.integers(-50, 0, N).astype(np.int64)),
        ("c1", "char1", rng.integers(65, 70, N).astype(np.uint8)),
        ("i32", "int32", rng.integers(-3, 9, N).astype(np.int32)),
        ("i64", "int64", (rng.integers(0, 11, N) * 1_000_003 - 5_000_000)
         .astype(np.int64)),
        ("c1b", "char1", rng.integers(0, 256, N).astype(np.uint8)),
        ("s0", "int32", rng.integers(0, 2, N).astype(np.int32)),
        ("s1", "int64", rng.choice([-3, 4], N).astype(np.int64)),
        ("cc0", "char1", rng.integers(65, 67, N).astype(np.uint8)),
        ("cc1", "char1", rng.integers(70, 73, N).astype(np.uint8)),
        ("w0", "int32", w0.astype(np.int32)),
        ("w1", "int64", w1.astype(np.int64)),
        ("k0", "int64", pool0[pick].astype(np.int64)),
        ("k1", "int64", pool1[pick].astype(np.int64)),
        ("e0", "int64", e0.astype(np.int64)),
        ("e1", "int64", e1.astype(np.int64)),
        ("e1x", "int64", e1x.astype(np.int64)),
        ("fk0", "int64", rng.integers(0, 320, N).astype(np.int64)),
        ("fk1", "int64", ((rng.integers(0, 270, N) - 130) * 1000 + 7)
         .astype(np.int64)),
    ]
    nullmap = {c: rng.random(N) < 0.2 for c in ("c1", "i32", "i64", "c1b")}
    return register(eng, "gk_drive", cols, nullmap)


@pytest.fixture(scope="module")
def builds(eng):
    """b0: dense keys 1..301 (index map); b1: sparse keys around zero
    (hash map).  Both carry nullable payload columns; b0.fk2 is a
    nullable probe key into b1."""
    rng = np.random.default_rng(2027)
    m0, m1 = 301, 257
    k1 = ((rng.permutation(np.arange(m1)) - m1 // 2) * 1000 + 7)
    assert k1.min() < 0 and k1.max() > 8 * m1 + 16
    b0 = register(eng, "gk_b0", [
        ("bk", "int64", rng.permutation(np.arange(1, m0 + 1)).astype(np.int64)),
        ("nat", "int32", rng.integers(-4, 21, m0).astype(np.int32)),
        ("keep", "int32", rng.integers(0, 10, m0).astype(np.int32)),
        ("fk2", "int64", rng.choice(np.concatenate([k1, k1 + 2]), m0)
         .astype(np.int64))],
        {"nat": rng.random(m0) < 0.15, "fk2": rng.random(m0) < 0.1})
    b1 = register(eng, "gk_b1", [
        ("bk", "int64", k1.astype(np.int64)),
        ("year", "int64", (1992 + rng.integers(0, 7, m1)).astype(np.int64)),
        ("keep", "int32", rng.integers(0, 10, m1).astype(np.int32))],
        {"year": rng.random(m1) < 0.15})
    return b0, b1


def test_int32_int64_pair_overflows_the_block_cache(eng, mode, drive):
    t, d, nl = drive
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["a32", "b64"], AGGS)
    pairs = {(g[0], g[1]) for g in exp}
    assert 2900 < len(pairs) <= 3000
    assert all(a < 0 and b < 0 for a, b in pairs)
    assert any((b, a) not in pairs for a, b in pairs)
    assert "path_plan_group_packed" in paths, paths


def test_char1_with_int_pairs_and_null_keys(eng, mode, drive):
    t, d, nl = drive
    for cols in (["c1", "i32"], ["i64", "c1b"]):
        _p, exp, paths = run(eng, mode, t, d, nl, [("v", 0, 90_000)], [],
                             cols, AGGS)
        pairs = {(g[0], g[1]) for g in exp}
        assert (NULL_KEY, NULL_KEY) in pairs
        assert any(a == NULL_KEY and b != NULL_KEY for a, b in pairs)
        assert any(a != NULL_KEY and b == NULL_KEY for a, b in pairs)
        assert "path_plan_group_packed" in paths, paths


def test_few_groups_bake_on_the_packed_code(eng, mode, drive):
    t, d, nl = drive
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["s0", "s1"], AGGS)
    assert [(g[0], g[1]) for g in exp] == [(0, -3), (0, 4), (1, -3), (1, 4)]
    assert "path_plan_group_packed" in paths, paths
    if mode == "rtc":
        assert any(s.startswith("path_plan_rtc_baked") for s in paths), paths
    # the (char1, char1) pair keeps its code and never shows the row
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["cc0", "cc1"], AGGS)
    assert len(exp) == 6
    assert "path_plan_group_packed" not in paths, paths
    if mode == "rtc":
        assert any(s.startswith("path_plan_rtc_baked") for s in paths), paths


def test_width_holds_the_null_code(eng, mode, drive):
    """both columns span exactly 2^K values and one row holds both
    maxima: K bits instead of K + 1 would carry column 1 into column 0"""
    t, d, nl = drive
    assert (d["w0"].min(), d["w0"].max()) == (M0, M0 + (1 << K) - 1)
    assert (d["w1"].min(), d["w1"].max()) == (M1, M1 + (1 << K) - 1)
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["w0", "w1"], AGGS)
    assert len(exp) == 1 << (2 * K)
    assert (exp[-1][0], exp[-1][1]) == (int(d["w0"].max()),
                                        int(d["w1"].max()))


def test_wide_values_narrow_range(eng, mode, drive):
    t, d, nl = drive
    assert d["k0"].min() == -(1 << 45) and d["k0"].max() == -(1 << 45) + 999
    assert d["k1"].min() == 1 << 50 and d["k1"].max() == (1 << 50) + 1999
    _p, exp, paths = run(eng, mode, t, d, nl, [], [], ["k0", "k1"], AGGS)
    assert 1400 < len(exp) <= 1500
    assert "path_plan_group_packed" in paths, paths


def test_both_keys_payload_of_two_inner_joins(eng, mode, drive, builds):
    """group by (b0.nat, b1.year), both nullable: join 0 probes a dense
    index map, join 1 a hash map, from the driving table and then
    chained through b0.fk2; both builds filter"""
    t, d, nl = drive
    (t0, d0, n0), (t1, d1, n1) = builds
    j0 = join(t0, d0, n0, "bk", "fk0", preds=[("keep", 1, 10)])
    for j1 in (join(t1, d1, n1, "bk", "fk1", preds=[("keep", 0, 8)]),
               join(t1, d1, n1, "bk", "fk2", preds=[("keep", 0, 8)],
                    probe_src=1)):
        _p, exp, paths = run(eng, mode, t, d, nl, [], [j0, j1],
                             [(0, "nat"), (1, "year")], AGGS)
        pairs = {(g[0], g[1]) for g in exp}
        assert len(pairs) > 30
        assert any(a == NULL_KEY for a, _b in pairs)
        assert any(b == NULL_KEY for _a, b in pairs)
        assert {"path_plan_join_index_dense", "path_plan_join_index_hash",
                "path_plan_group_packed"} <= paths, paths


def test_budget_edge(eng, mode, drive):
    """31 + 31 bits are exact; one maximum one larger is 31 + 32, refused
    with GG_ENOTSUP at compile or at the first execute, and the engine
    runs the next plan"""
    from greengage_amd import EngineError
    t, d, nl = drive
    _p, exp, _paths = run(eng, mode, t, d, nl, [], [], ["e0", "e1"], AGGS)
    assert [(g[0], g[1]) for g in exp] == [(0, 0), (0, EDGE), (EDGE, 0),
                                           (EDGE, EDGE)]
    with plan_mode(mode), pytest.raises(EngineError) as ei:
        p = eng.compile_plan(t, group_cols=["e0", "e1x"], aggs=AGGS)
        eng.execute_plan(p, max_groups=16)
    assert ENOTSUP in str(ei.value), ei.value
    assert "31 + 32 bits" in str(ei.value), ei.value
    run(eng, mode, t, d, nl, [], [], ["e1", "e0"], AGGS, repeats=1)
