"""Directed cases for INNER joins with payload columns in compiled plans.

Every case is compared bit-exactly with the evaluator of
plan_payload_ref and, unless its docstring says otherwise, runs on the
default path (hipRTC-generated kernels) and with GG_PLAN_RTC=0 (the
interpreted kernel of plan.hip), three executes each, so plans with at
most 8 groups run the baked kernel on executes 2 and 3.

Driving tables hold 6,000-20,000 rows, build tables 257-2,000 rows,
never a multiple of 64 or 256.  The cases aim at what a key -> row
index join can get wrong: the dense and the hash map, gathers through
the index for group keys, factors, NULL flags and chained probe keys,
probe keys outside the map (negative, past its end, INT64_MIN),
builds that keep nothing, and the uniqueness rule.
"""
import numpy as np
import pytest

import plan_minmax_ref
from plan_payload_ref import (NEG_INF, NotUnique, eval_plan, join, register,
                              run, strip)

pytestmark = pytest.mark.gpu

I64_MIN = -(1 << 63)
EINVAL, ENOTSUP = "status 1:", "status 5:"


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


def dense_keys(rng, m):
    return rng.permutation(np.arange(1, m + 1)).astype(np.int64)


def sparse_keys(rng, m):
    """key*1000+7 around zero: negative keys, max > 8*rows+16"""
    k = (rng.permutation(np.arange(m)) - m // 2) * 1000 + 7
    assert k.min() < 0 and k.max() > 8 * m + 16
    return k.astype(np.int64)


def mk_build(eng, name, rng, keys, ktype="int64", nullmap=None, fk2=None):
    m = len(keys)
    cols = [("bk", ktype, keys.astype(np.int32 if ktype == "int32"
                                      else np.int64)),
            ("rowid", "int64", np.arange(m, dtype=np.int64)),
            ("cat", "int32", rng.integers(0, 7, m).astype(np.int32)),
            ("disc", "int64", rng.integers(0, 11, m).astype(np.int64)),
            ("w", "int32", rng.integers(-500, 500, m).astype(np.int32)),
            ("flag", "char1", rng.integers(65, 68, m).astype(np.uint8))]
    if fk2 is not None:
        cols.append(("fk2", "int64", fk2.astype(np.int64)))
    return register(eng, name, cols, nullmap)


def mk_drive(eng, name, rng, fk, ktype="int64", nullmap=None):
    n = len(fk)
    cols = [("fk", ktype, fk.astype(np.int32 if ktype == "int32"
                                    else np.int64)),
            ("price", "int64",
             rng.integers(-1000, 100000, n).astype(np.int64)),
            ("qty", "int32", rng.integers(1, 51, n).astype(np.int32)),
            ("st", "char1", rng.integers(70, 73, n).astype(np.uint8)),
            ("g", "int32", rng.integers(0, 5, n).astype(np.int32))]
    return register(eng, name, cols, nullmap)


AGGS5 = [("sum", [("price", "id")]), "count", ("min", ("price", "id")),
         ("max", ("qty", "id")), ("avg", [("price", "id")])]


def test_dense_group_by_payload(eng, mode):
    rng = np.random.default_rng(11)
    m, n = 1000, 12_345
    keys = dense_keys(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_dense_b_{mode}", rng, keys)
    t, d, nl = mk_drive(eng, f"pp_dense_d_{mode}", rng, rng.choice(keys, n))
    j = join(bt, bd, bn, "bk", "fk")
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j], [(0, "cat")], AGGS5)
    assert len(exp) == 7 and sum(g[2][1] for g in exp) == n
    assert "path_plan_join_index_dense" in paths, paths
    assert "path_plan_join_index_hash" not in paths, paths


@pytest.mark.parametrize("ktype", ["int64", "int32"])
def test_hash_group_by_payload(eng, mode, ktype):
    rng = np.random.default_rng(12)
    m, n = 1021, 12_345
    if ktype == "int64":
        keys = sparse_keys(rng, m)
    else:
        keys = ((rng.permutation(np.arange(m)) - m // 2) * 3 + 1)
        assert keys.min() < 0
    bt, bd, bn = mk_build(eng, f"pp_hash_b_{mode}_{ktype}", rng, keys, ktype)
    t, d, nl = mk_drive(eng, f"pp_hash_d_{mode}_{ktype}", rng,
                        rng.choice(keys, n), ktype)
    j = join(bt, bd, bn, "bk", "fk")
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j], [(0, "cat")], AGGS5)
    assert len(exp) == 7 and sum(g[2][1] for g in exp) == n
    assert "path_plan_join_index_hash" in paths, paths
    assert "path_plan_join_index_dense" not in paths, paths


@pytest.mark.parametrize("grouped", [False, True])
def test_payload_as_aggregate_factor(eng, mode, grouped):
    """SUM(driving.price * (100 - build.disc)) and MAX(build.w)"""
    rng = np.random.default_rng(13)
    m, n = 777, 9_001
    keys = dense_keys(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_fac_b_{mode}_{grouped}", rng, keys)
    t, d, nl = mk_drive(eng, f"pp_fac_d_{mode}_{grouped}", rng,
                        rng.choice(keys, n))
    j = join(bt, bd, bn, "bk", "fk")
    aggs = [("sum", [("price", "id"), ((0, "disc"), "sub100")]),
            ("max", ((0, "w"), "id")), ("count", (0, "disc")),
            ("avg", [((0, "w"), "add100"), ("qty", "id")])]
    run(eng, mode, t, d, nl, [("qty", 5, 45)], [j],
        ["g"] if grouped else [], aggs)


def test_two_char1_keys_from_different_sources(eng, mode):
    rng = np.random.default_rng(14)
    m, n = 513, 8_191
    keys = sparse_keys(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_c1_b_{mode}", rng, keys)
    t, d, nl = mk_drive(eng, f"pp_c1_d_{mode}", rng, rng.choice(keys, n))
    j = join(bt, bd, bn, "bk", "fk")
    aggs = ["count", ("sum", [("qty", "id"), ((0, "disc"), "id")])]
    _p, exp, _ = run(eng, mode, t, d, nl, [], [j], ["st", (0, "flag")], aggs)
    assert len(exp) == 9
    _p, exp, _ = run(eng, mode, t, d, nl, [], [j], [(0, "flag"), "st"], aggs)
    assert len(exp) == 9


@pytest.mark.parametrize("keys_of", [dense_keys, sparse_keys])
def test_nulls_everywhere(eng, mode, keys_of):
    rng = np.random.default_rng(15)
    m, n = 999, 10_007
    keys = keys_of(rng, m)
    bnull = {"bk": rng.random(m) < 0.1, "cat": rng.random(m) < 0.15,
             "w": rng.random(m) < 0.2}
    bt, bd, bn = mk_build(eng, f"pp_null_b_{mode}_{keys_of.__name__}", rng,
                          keys, nullmap=bnull)
    # every build row of category 3 has a NULL w: that group's MIN is NULL
    bn["w"] |= (bd["cat"] == 3) & ~bn["cat"]
    eng.set_nulls(bt, "w", bn["w"].astype(np.uint8))
    t, d, nl = mk_drive(eng, f"pp_null_d_{mode}_{keys_of.__name__}", rng,
                        rng.choice(keys, n),
                        nullmap={"fk": rng.random(n) < 0.1,
                                 "price": rng.random(n) < 0.1})
    j = join(bt, bd, bn, "bk", "fk")
    aggs = ["count", ("min", ((0, "w"), "id")), ("count", (0, "w")),
            ("sum", [("price", "id"), ((0, "w"), "add100")])]
    _p, exp, _ = run(eng, mode, t, d, nl, [], [j], [(0, "cat")], aggs)
    byk = {g[0]: g[2] for g in exp}
    # the NULL group exists only through NULL payload keys
    assert plan_minmax_ref.NULL_KEY in byk and len(exp) == 8
    assert byk[3][0] > 0 and byk[3][1] is None and byk[3][2] == 0
    # NULL probe keys and NULL build keys matched nothing
    assert sum(v[0] for v in byk.values()) < n * 0.9
    run(eng, mode, t, d, nl, [], [j], [], aggs)


@pytest.mark.parametrize("kind1", ["semi", "inner"])
def test_chain(eng, mode, kind1):
    """driving -> A (payload a.fk2) -> B: join 1 probes with A's column.
    SEMI with build predicates = "orders of customers in one segment";
    INNER grouped by a B column = "by nation"."""
    rng = np.random.default_rng(16)
    mb, ma, n = 257, 1_999, 15_001
    bkeys = sparse_keys(rng, mb)
    akeys = dense_keys(rng, ma)
    btab, bd, bn = mk_build(eng, f"pp_ch_b_{mode}_{kind1}", rng, bkeys,
                            nullmap={"cat": rng.random(mb) < 0.1})
    # a tenth of A's rows point at no B row, some have a NULL pointer
    fk2 = np.where(rng.random(ma) < 0.1, 5, rng.choice(bkeys, ma))
    atab, ad, an = mk_build(eng, f"pp_ch_a_{mode}_{kind1}", rng, akeys,
                            nullmap={"fk2": rng.random(ma) < 0.05}, fk2=fk2)
    t, d, nl = mk_drive(eng, f"pp_ch_d_{mode}_{kind1}", rng,
                        rng.integers(-20, ma + 40, n))
    j0 = join(atab, ad, an, "bk", "fk")
    if kind1 == "semi":
        j1 = join(btab, bd, bn, "bk", "fk2", kind="semi", probe_src=1,
                  preds=[("flag", 66, 67)])
        group = [(0, "cat")]
        aggs = ["count", ("sum", [("price", "id"), ((0, "disc"), "sub100")])]
    else:
        j1 = join(btab, bd, bn, "bk", "fk2", probe_src=1)
        group = [(1, "cat")]
        aggs = ["count", ("max", ((0, "w"), "id")),
                ("sum", [((1, "disc"), "id"), ((0, "disc"), "add100"),
                         ("qty", "id")])]
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j0, j1], group, aggs)
    total = sum(g[2][0] for g in exp)
    assert 0 < total < n
    assert "path_plan_join_index_dense" in paths, paths
    assert ("path_plan_join_hash" if kind1 == "semi"
            else "path_plan_join_index_hash") in paths, paths
    run(eng, mode, t, d, nl, [], [j0, j1], [], aggs)


@pytest.mark.parametrize("order", ["semi_first", "inner_first"])
def test_mixed_semi_and_inner(eng, mode, order):
    rng = np.random.default_rng(17)
    m, n = 1_003, 11_111
    ikeys, skeys = dense_keys(rng, m), sparse_keys(rng, 600)
    it, idt, inl = mk_build(eng, f"pp_mix_i_{mode}_{order}", rng, ikeys)
    stab, sd, sn = mk_build(eng, f"pp_mix_s_{mode}_{order}", rng,
                            np.concatenate([skeys, skeys[:50]]))
    # sfk: half the SEMI probe keys have no partner
    t, d, nl = register(eng, f"pp_mix_d_{mode}_{order}", [
        ("fk", "int64", rng.choice(ikeys, n)),
        ("sfk", "int64", rng.choice(np.concatenate([skeys, skeys + 1]), n)),
        ("price", "int64", rng.integers(-1000, 100000, n).astype(np.int64)),
        ("qty", "int32", rng.integers(1, 51, n).astype(np.int32))])
    ji = join(it, idt, inl, "bk", "fk")
    js = join(stab, sd, sn, "bk", "sfk", kind="semi",
              preds=[("cat", 0, 5)])
    k = 1 if order == "semi_first" else 0
    joins = [js, ji] if order == "semi_first" else [ji, js]
    aggs = ["count", ("sum", [("price", "id"), ((k, "disc"), "sub100")]),
            ("min", ((k, "w"), "id"))]
    _p, exp, paths = run(eng, mode, t, d, nl, [], joins, [(k, "cat")], aggs)
    assert 0 < sum(g[2][0] for g in exp) < n
    assert {"path_plan_join_index_dense", "path_plan_join_hash"} <= paths


@pytest.mark.parametrize("keys_of", [dense_keys, sparse_keys])
def test_same_table_joined_twice(eng, mode, keys_of):
    """one build table behind two INNER joins with different probe keys
    (two FKs into one dimension): the same nullable column read through
    both sources is two different values per row, for the loaded factor
    and for the non-NULL counts behind AVG and MIN alike"""
    rng = np.random.default_rng(27)
    m, n = 901, 9_003
    keys = keys_of(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_twice_b_{mode}_{keys_of.__name__}", rng,
                          keys, nullmap={"w": rng.random(m) < 0.3,
                                         "disc": rng.random(m) < 0.2})
    t, d, nl = register(eng, f"pp_twice_d_{mode}_{keys_of.__name__}", [
        ("fa", "int64", rng.choice(keys, n)),
        ("fb", "int64", rng.choice(keys, n)),
        ("qty", "int32", rng.integers(1, 51, n).astype(np.int32)),
        ("g", "int32", rng.integers(0, 4, n).astype(np.int32))])
    ja = join(bt, bd, bn, "bk", "fa")
    jb = join(bt, bd, bn, "bk", "fb")
    aggs = [("sum", [((0, "w"), "id")]), ("sum", [((1, "w"), "id")]),
            ("avg", [((0, "w"), "id")]), ("min", ((1, "w"), "id")),
            ("sum", [((0, "disc"), "id"), ((1, "disc"), "sub100"),
                     ("qty", "id")])]
    for group in (["g"], [(1, "cat")], []):
        _p, exp, _ = run(eng, mode, t, d, nl, [], [ja, jb], group, aggs)
        # the two sources really differ, so sharing a load or a count
        # between them cannot pass
        assert any(g[2][0] != g[2][1] for g in exp)
    _p, exp, _ = run(eng, mode, t, d, nl, [], [ja, jb], [],
                     [("count", (0, "w")), ("count", (1, "w")),
                      ("avg", [((0, "w"), "id")]),
                      ("max", ((1, "w"), "add100"))])
    c0, c1, avg0, _mx = exp[0][2]
    assert c0 != c1 and avg0[1] == c0


def test_probe_misses_dense(eng, mode):
    """half the probe keys have no build row: keys below 0, keys inside
    the map whose build row is filtered out or absent, keys past dlen"""
    rng = np.random.default_rng(18)
    m, n = 1_001, 14_003
    keys = rng.permutation(np.arange(1, 2 * m + 1, 2)).astype(np.int64)
    bt, bd, bn = mk_build(eng, f"pp_miss_b_{mode}", rng, keys)
    fk = rng.integers(-300, 3 * m, n)
    fk[:4] = [-1, 0, 2 * m, 1 << 40]
    t, d, nl = mk_drive(eng, f"pp_miss_d_{mode}", rng, fk)
    j = join(bt, bd, bn, "bk", "fk", preds=[("w", -400, 400)])
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j], [(0, "cat")], AGGS5)
    hit = sum(g[2][1] for g in exp)
    assert n * 0.15 < hit < n * 0.6
    assert "path_plan_join_index_dense" in paths, paths


def test_probe_misses_hash(eng, mode):
    """... and on the hash path, where a probe key of INT64_MIN encodes
    as the empty-slot sentinel and must find nothing"""
    rng = np.random.default_rng(19)
    m, n = 1_001, 14_003
    keys = sparse_keys(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_missh_b_{mode}", rng, keys)
    fk = np.where(rng.random(n) < 0.5, rng.choice(keys, n),
                  rng.choice(keys, n) + rng.integers(1, 900, n))
    fk[::97] = I64_MIN
    t, d, nl = mk_drive(eng, f"pp_missh_d_{mode}", rng, fk)
    j = join(bt, bd, bn, "bk", "fk")
    _p, exp, paths = run(eng, mode, t, d, nl, [], [j], [(0, "cat")], AGGS5)
    hit = sum(g[2][1] for g in exp)
    assert n * 0.4 < hit < n * 0.6
    assert "path_plan_join_index_hash" in paths, paths
    # as a global group: no row may come from the INT64_MIN probes
    _p, exp, _ = run(eng, mode, t, d, nl, [("fk", NEG_INF, I64_MIN + 1)],
                     [j], [], ["count", ("max", ((0, "w"), "id"))])
    assert exp == [(0, 0, [0, None])]


@pytest.mark.parametrize("keys_of", [dense_keys, sparse_keys])
def test_build_keeps_nothing(eng, mode, keys_of):
    rng = np.random.default_rng(20)
    m, n = 300, 6_007
    keys = keys_of(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_none_b_{mode}_{keys_of.__name__}", rng,
                          keys)
    t, d, nl = mk_drive(eng, f"pp_none_d_{mode}_{keys_of.__name__}", rng,
                        rng.choice(keys, n))
    j = join(bt, bd, bn, "bk", "fk", preds=[("w", 1000, 1001)])
    aggs = ["count", ("sum", [("price", "id")]), ("min", ((0, "w"), "id")),
            ("avg", [((0, "disc"), "id")])]
    _p, exp, _ = run(eng, mode, t, d, nl, [], [j], [(0, "cat")], aggs)
    assert exp == []
    _p, exp, _ = run(eng, mode, t, d, nl, [], [j], [], aggs)
    assert exp == [(0, 0, [0, 0, None, (0, 0)])]


def test_both_scan_loops(eng):
    """4*2048*256 + 777 driving rows: the smallest table at which the
    interpreted kernel's 4-way strided loop runs as well as its tail.
    Generated kernels, two executes; one interpreted execute on top."""
    rng = np.random.default_rng(21)
    m, n = 1_000, 4 * 2048 * 256 + 777
    keys = ((rng.permutation(np.arange(m)) - 100) * 5 + 2).astype(np.int32)
    bt, bd, bn = register(eng, "pp_big_b", [
        ("bk", "int32", keys),
        ("cat", "int32", rng.integers(0, 6, m).astype(np.int32))])
    fk = rng.integers(-600, 5 * m, n).astype(np.int32)
    t, d, nl = register(eng, "pp_big_d", [
        ("fk", "int32", fk),
        ("v", "int32", rng.integers(-9, 1000, n).astype(np.int32))])
    j = join(bt, bd, bn, "bk", "fk")
    aggs = [("sum", [("v", "id")])]
    exp = eval_plan(n, d, nl, [], [j], [(0, "cat")], aggs)
    assert len(exp) == 6
    run(eng, "rtc", t, d, nl, [], [j], [(0, "cat")], aggs, repeats=2,
        exp=exp)
    run(eng, "interp", t, d, nl, [], [j], [(0, "cat")], aggs, repeats=1,
        exp=exp)


def test_fast_tier_with_short_build_side(eng, mode):
    """non-negative bounded factors, one a payload column of a build
    table 60x shorter than the driving table: the overflow proof bounds
    it over the build table's own rows and the plan reaches the one-word
    baked tier; a single negative payload value must keep it off."""
    rng = np.random.default_rng(22)
    m, n = 300, 18_001
    keys = dense_keys(rng, m)
    fk = rng.choice(keys, n)
    base = rng.integers(0, 11, m).astype(np.int64)
    for tag, disc in (("pos", base), ("neg", np.where(
            np.arange(m) == 7, -3, base))):
        bt, bd, bn = register(eng, f"pp_fast_b_{mode}_{tag}", [
            ("bk", "int64", keys), ("disc", "int64", disc)])
        t, d, nl = register(eng, f"pp_fast_d_{mode}_{tag}", [
            ("fk", "int64", fk),
            ("qty", "int64", rng.integers(1, 51, n).astype(np.int64)),
            ("st", "char1", rng.integers(70, 73, n).astype(np.uint8))])
        j = join(bt, bd, bn, "bk", "fk")
        aggs = ["count", ("sum", [("qty", "id"), ((0, "disc"), "id")]),
                ("sum", [("qty", "id"), ((0, "disc"), "sub100")])]
        _p, exp, paths = run(eng, mode, t, d, nl, [], [j], ["st"], aggs)
        assert len(exp) == 3
        if tag == "pos":
            assert paths & {"path_plan_rtc_baked_fast", "path_plan_interp"}
            if "path_plan_rtc" in paths:
                assert "path_plan_rtc_baked_fast" in paths, paths
        else:
            assert "path_plan_rtc_baked_fast" not in paths, paths
            if "path_plan_rtc" in paths:
                assert "path_plan_rtc_baked" in paths, paths


@pytest.mark.parametrize("keys_of", [dense_keys, sparse_keys])
def test_duplicate_build_key_is_refused(eng, mode, keys_of):
    """first and last build row share a key: GG_ENOTSUP from execute on
    both map layouts; fine once a build predicate removes one of the
    pair, and fine for a SEMI join"""
    from greengage_amd import EngineError
    from plan_minmax_ref import plan_mode
    rng = np.random.default_rng(23)
    m, n = 1_931, 7_001
    keys = keys_of(rng, m)
    keys[-1] = keys[0]
    bt, bd, bn = mk_build(eng, f"pp_dup_b_{mode}_{keys_of.__name__}", rng,
                          keys)
    t, d, nl = mk_drive(eng, f"pp_dup_d_{mode}_{keys_of.__name__}", rng,
                        rng.choice(keys, n))
    aggs = ["count", ("sum", [("price", "id")])]
    dup = join(bt, bd, bn, "bk", "fk")
    with pytest.raises(NotUnique):
        eval_plan(n, d, nl, [], [dup], [(0, "cat")], aggs)
    with plan_mode(mode):
        p = eng.compile_plan(t, joins=strip([dup]), group_cols=[(0, "cat")],
                             aggs=aggs)
        for _ in range(2):
            with pytest.raises(EngineError, match=ENOTSUP):
                eng.execute_plan(p)
    paths = {s["name"] for s in eng.stats(p)}
    assert ("path_plan_join_index_dense" if keys_of is dense_keys
            else "path_plan_join_index_hash") in paths, paths
    # the duplicate fails the build predicate: unique among passing rows
    ok = join(bt, bd, bn, "bk", "fk", preds=[("rowid", 0, m - 1)])
    run(eng, mode, t, d, nl, [], [ok], [(0, "cat")], aggs)
    semi = join(bt, bd, bn, "bk", "fk", kind="semi")
    run(eng, mode, t, d, nl, [], [semi], ["g"], aggs)


def test_duplicate_null_keys_do_not_count(eng, mode):
    rng = np.random.default_rng(24)
    m, n = 601, 6_001
    keys = dense_keys(rng, m)
    knull = np.zeros(m, bool)
    knull[[0, m - 1]] = True
    keys[m - 1] = keys[0]
    bt, bd, bn = mk_build(eng, f"pp_dupn_b_{mode}", rng, keys,
                          nullmap={"bk": knull})
    t, d, nl = mk_drive(eng, f"pp_dupn_d_{mode}", rng, rng.choice(keys, n))
    run(eng, mode, t, d, nl, [], [join(bt, bd, bn, "bk", "fk")],
        [(0, "cat")], ["count", ("sum", [((0, "disc"), "id")])])


def test_compile_time_rejections(eng):
    from greengage_amd import EngineError
    rng = np.random.default_rng(25)
    keys = dense_keys(rng, 257)
    bt, bd, bn = mk_build(eng, "pp_rej_b", rng, keys, fk2=keys)
    t, _d, _nl = mk_drive(eng, "pp_rej_d", rng, rng.choice(keys, 6_000))
    inner = {"table": bt, "build_key": "bk", "probe_key": "fk",
             "kind": "inner"}
    semi = dict(inner, kind="semi")
    chained = dict(inner, probe_key="fk2")

    def rejects(field, **kw):
        kw.setdefault("aggs", ["count"])
        with pytest.raises(EngineError, match=EINVAL) as ei:
            eng.compile_plan(t, **kw)
        assert field in str(ei.value), ei.value

    # a source naming a SEMI join
    rejects("group_src", joins=[semi], group_cols=[(0, "cat")])
    rejects("agg src", joins=[semi], aggs=[("sum", [((0, "disc"), "id")])])
    rejects("probe_src", joins=[semi, dict(chained, probe_src=1)])
    # forward and self probe_src
    rejects("probe_src", joins=[dict(chained, probe_src=2), inner])
    rejects("probe_src", joins=[dict(chained, probe_src=1)])
    # a source past the plan's joins
    rejects("group_src", joins=[inner], group_cols=[(1, "cat")])
    rejects("agg src", joins=[inner], aggs=[("max", ((2, "w"), "id"))])
    rejects("group_src", group_cols=[(0, "cat")])
    # a payload column the build table does not have
    rejects("column missing", joins=[inner], group_cols=[(0, "nope")])
    rejects("column missing", joins=[inner],
            aggs=[("sum", [((0, "price"), "id")])])
    # the accepted forms of the same descriptors still compile
    eng.compile_plan(t, joins=[inner, dict(chained, probe_src=1)],
                     group_cols=[(1, "cat")],
                     aggs=[("max", ((0, "w"), "id"))])


def test_unchanged_semi_plan(eng, mode):
    """a descriptor written without any of the new keys means what it
    meant: checked against the older evaluator"""
    rng = np.random.default_rng(26)
    m, n = 700, 9_999
    keys = dense_keys(rng, m)
    bt, bd, bn = mk_build(eng, f"pp_old_b_{mode}", rng,
                          np.concatenate([keys, keys[:90]]))
    t, d, nl = mk_drive(eng, f"pp_old_d_{mode}", rng,
                        rng.integers(-5, 2 * m, n))
    j = {"table": bt, "build_key": "bk", "probe_key": "fk",
         "preds": [("cat", 1, 6)], "_n": len(bd["bk"]), "_data": bd,
         "_nulls": bn}
    aggs = ["count", ("sum", [("price", "id"), ("qty", "sub100")]),
            ("min", ("price", "id"))]
    exp = plan_minmax_ref.eval_plan(n, d, nl, [("qty", 3, 40)], [j], ["g"],
                                    aggs)
    assert len(exp) == 5
    with plan_minmax_ref.plan_mode(mode):
        p = eng.compile_plan(
            t, preds=[("qty", 3, 40)],
            joins=[{"table": bt, "build_key": "bk", "probe_key": "fk",
                    "preds": [("cat", 1, 6)]}],
            group_cols=["g"], aggs=aggs)
        for _ in range(3):
            assert sorted(eng.execute_plan(p)) == exp
    paths = {s["name"] for s in eng.stats(p)}
    assert "path_plan_join_bitmap" in paths
    assert not paths & {"path_plan_join_index_dense",
                        "path_plan_join_index_hash"}
