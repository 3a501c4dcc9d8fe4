"""LEFT OUTER and ANTI joins of compiled plans (engine_abi.h GG_JOIN_LEFT /
GG_JOIN_ANTI), directed cases.

Every case runs on the generated kernels and, under plan_mode("interp"),
on the interpreted kernel, three executes each (the baked kernel takes
over from the second where one is made), and must equal
plan_outer_ref.eval_plan bit for bit.

Shapes are the smallest at which the kernels can still go wrong: driving
rows n in {1, 257, 6001} (one thread; a second block holding one row;
several blocks) and build rows m in {3, 601} (a build table far smaller
than any stray index; one of several blocks).  The row loop body is the
same in the 4-row main loop and the tail, so no case needs the ~2.1 M rows
at which the interpreted kernel's main loop engages.
"""
import ctypes

import numpy as np
import pytest

from plan_outer_ref import (NEG_INF, NULL_KEY, POS_INF, eval_plan, join,
                            register, run)

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = 1, 5
NS = [1, 257, 6001]
MS = [3, 601]
INT64_MIN = -(1 << 63)


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


def _keys(rng, m, style, unique=True):
    """build keys: `dense` takes the index map / bitmap, `sparse` (int64)
    and `int32` hash"""
    base = rng.permutation(np.arange(2 * m))[:m]
    if not unique:
        base[m // 2:] = base[:m - m // 2]
    if style == "dense":
        return "int64", (base + 1).astype(np.int64)
    if style == "sparse":
        return "int64", ((base - m) * 1000 + 7).astype(np.int64)
    return "int32", ((base - m) * 3 + 1).astype(np.int32)


def _build(eng, name, rng, m, style, nullmap=None, unique=True, extra=()):
    ktype, keys = _keys(rng, m, style, unique)
    cols = [("bk", ktype, keys),
            ("w", "int32", rng.integers(-50, 50, m).astype(np.int32)),
            ("v", "int64", rng.integers(0, 1000, m).astype(np.int64)),
            ("c", "char1", rng.integers(0, 3, m).astype(np.uint8)),
            ("s", "int32", rng.integers(-2, 2, m).astype(np.int32))]
    cols += list(extra)
    return (keys.astype(np.int64),) + register(eng, name, cols, nullmap)


def _probe(rng, keys, n, style, present_only=False):
    """probe keys: present ones, absent ones inside the key range,
    negative ones and ones past the dense map; INT64_MIN where the join
    hashes (it encodes as the hash map's empty sentinel)"""
    if present_only:
        return rng.choice(keys, n)
    m = len(keys)
    absent = np.setdiff1d(np.arange(int(keys.min()), int(keys.max()) + 1),
                          keys)[:m]
    far = [-1, -7, int(keys.max()) + 1, int(keys.max()) + 64, 1 << 40]
    if style != "dense":
        far.append(INT64_MIN)
    pool = np.concatenate([keys, keys, absent, np.array(far, np.int64)])
    out = rng.choice(pool, n)
    # the edge keys are present whenever there is room for them
    k = min(len(far), n // 2)
    out[n - k:] = far[len(far) - k:]
    return out.astype(np.int64)


def _drive(eng, name, rng, n, fk, nullmap=None, extra=()):
    cols = [("x", "int32", rng.integers(-100, 100, n).astype(np.int32)),
            ("y", "int64", rng.integers(0, 50, n).astype(np.int64)),
            ("g", "char1", rng.integers(0, 3, n).astype(np.uint8)),
            ("fk", "int64", fk)]
    cols += list(extra)
    return register(eng, name, cols, nullmap)


# COUNT(*), COUNT(payload), SUM / MIN / MAX over payload factors, AVG over
# a driving x payload product: 8 accumulator slots
AGGS_P = ["count", ("count", (0, "w")), ("sum", [((0, "v"), "id")]),
          ("min", ((0, "w"), "id")), ("max", ((0, "w"), "sub100")),
          ("avg", [("x", "id"), ((0, "v"), "add100")])]
# the mixed product as a SUM, beside AVG and MAX of payload columns
AGGS_D = ["count", ("sum", [("x", "id"), ((0, "w"), "id")]),
          ("avg", [((0, "v"), "id")]), ("max", ((0, "v"), "id"))]


def _check_paths(paths, mode, left=0, anti=0):
    assert ("path_plan_interp" if mode == "interp" else "path_plan_rtc") \
        in paths
    assert ("path_plan_join_left" in paths) == bool(left)
    assert ("path_plan_join_anti" in paths) == bool(anti)


@pytest.mark.parametrize("style", ["dense", "sparse", "int32"])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_left_join(eng, mode, n, m, style):
    rng = np.random.default_rng(1000 + 10 * n + m)
    tag = f"{style}_{n}_{m}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, m, style,
                              {"w": rng.random(m) < 0.2})
    fk = _probe(rng, keys, n, style)
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n, fk,
                            {"fk": rng.random(n) < 0.1} if n > 1 else None)
    joins = [join(bt, bd, bn, "bk", "fk", kind="left")]
    # grouped by a payload column: the NULL-extended rows form a group
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins, [(0, "c")],
                         AGGS_P)
    _check_paths(paths, mode, left=1)
    assert ("path_plan_join_index_dense" if style == "dense"
            else "path_plan_join_index_hash") in paths
    assert sum(v[0] for _a, _b, v in exp) == n  # LEFT drops nothing
    if n > 1:
        assert exp[0][0] == NULL_KEY and 0 < exp[0][2][0] < n
        assert exp[0][2][1:5] == [0, 0, None, None]
        # ... by a driving column, and without one
        run(eng, mode, t, data, nulls, [("y", 5, POS_INF)], joins, ["g"],
            AGGS_D)
        _p, one, _paths = run(eng, mode, t, data, nulls, [], joins, [],
                              AGGS_P)
        assert one[0][2][0] == n and 0 < one[0][2][1] < n


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("style", ["dense", "sparse"])
def test_left_no_build_row_passes(eng, mode, n, style):
    """an ON-clause nothing satisfies: every row is NULL-extended, none is
    dropped"""
    rng = np.random.default_rng(1100 + n)
    tag = f"none_{style}_{n}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, 601, style)
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, keys, n, style, present_only=True))
    joins = [join(bt, bd, bn, "bk", "fk", kind="left",
                  preds=[("v", 5000, POS_INF)])]
    aggs = ["count", ("count", (0, "w")), ("sum", [((0, "v"), "id")]),
            ("max", ((0, "w"), "id"))]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins, [(0, "c")],
                         aggs)
    assert exp == [(NULL_KEY, 0, [n, 0, 0, None])]
    _check_paths(paths, mode, left=1)
    _p, exp, _paths = run(eng, mode, t, data, nulls, [], joins, [], aggs)
    assert exp == [(0, 0, [n, 0, 0, None])]


@pytest.mark.parametrize("style", ["dense", "int32"])
def test_left_where_every_row_matches_is_inner(eng, mode, style):
    rng = np.random.default_rng(1200)
    n, m = 6001, 601
    tag = f"all_{style}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, m, style,
                              {"w": rng.random(m) < 0.2})
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, keys, n, style, present_only=True))
    inner = eval_plan(n, data, nulls, [], [join(bt, bd, bn, "bk", "fk",
                                                kind="inner")],
                      [(0, "c")], AGGS_P)
    _p, exp, paths = run(eng, mode, t, data, nulls, [],
                         [join(bt, bd, bn, "bk", "fk", kind="left")],
                         [(0, "c")], AGGS_P)
    assert exp == inner and len(exp) == 3
    _check_paths(paths, mode, left=1)


@pytest.mark.parametrize("n", [257, 6001])
def test_left_payload_group_pairs(eng, mode, n):
    """both columns of a packed pair, and one column of a char1 pair, from
    a LEFT source; the payload column has NULL flags of its own, which
    land in the same NULL group as the NULL extension"""
    rng = np.random.default_rng(1300 + n)
    m = 601
    tag = f"pair_{n}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, m, "dense",
                              {"c": rng.random(m) < 0.2,
                               "s": rng.random(m) < 0.2})
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, keys, n, "dense"))
    joins = [join(bt, bd, bn, "bk", "fk", kind="left")]
    aggs = ["count", ("count", (0, "c")), ("sum", [((0, "v"), "id")])]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins,
                         [(0, "s"), (0, "w")], aggs)
    assert "path_plan_group_packed" in paths
    both = [v for k0, k1, v in exp if k0 == NULL_KEY and k1 == NULL_KEY]
    assert len(both) == 1 and both[0][0] > 0
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins,
                         [(0, "c"), "g"], aggs)
    assert "path_plan_group_packed" not in paths
    # flag NULLs and NULL extension share the group: its COUNT(*) exceeds
    # the NULL-extended rows, its COUNT(c) is 0
    ext = eval_plan(n, data, nulls, [], joins, [], ["count",
                                                    ("count", (0, "bk"))])
    n_ext = ext[0][2][0] - ext[0][2][1]
    ng = [v for k0, _k1, v in exp if k0 == NULL_KEY]
    assert ng and sum(v[0] for v in ng) > n_ext > 0
    assert all(v[1] == 0 for v in ng)
    _p, exp, _paths = run(eng, mode, t, data, nulls, [], joins, [(0, "c")],
                          aggs)
    assert exp[0][0] == NULL_KEY and exp[0][2][0] > n_ext


@pytest.mark.parametrize("style", ["dense", "sparse"])
def test_filter_on_left_payload(eng, mode, style):
    """one filter with a LEFT-payload conjunct shared by two aggregates,
    another mixing a driving and a nullable payload column"""
    rng = np.random.default_rng(1400)
    n, m = 6001, 601
    tag = f"flt_{style}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, m, style,
                              {"w": rng.random(m) < 0.2})
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, keys, n, style))
    joins = [join(bt, bd, bn, "bk", "fk", kind="left")]
    f0 = [((0, "v"), 100, 900)]
    f1 = [("y", 10, POS_INF), ((0, "w"), NEG_INF, 20)]
    aggs = [flt("count", f0), flt(("sum", [("x", "id")]), f0), "count",
            flt(("sum", [("x", "id"), ((0, "v"), "id")]), f1),
            flt(("count", "y"), f1)]
    for group in ([], ["g"], [(0, "c")]):
        _p, exp, paths = run(eng, mode, t, data, nulls, [], joins, group,
                             aggs)
        _check_paths(paths, mode, left=1)
    null_group = exp[0]
    assert null_group[0] == NULL_KEY
    assert null_group[2][0] == 0 and null_group[2][2] > 0
    assert null_group[2][4] == 0


@pytest.mark.parametrize("style", ["dense", "sparse", "int32"])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_anti_join(eng, mode, n, m, style):
    """NOT EXISTS over duplicate build keys, NULL build keys (never match),
    NULL probe keys (survive) and build predicates"""
    rng = np.random.default_rng(1500 + 10 * n + m)
    tag = f"anti_{style}_{n}_{m}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, m, style,
                              {"bk": rng.random(m) < 0.25}, unique=False)
    fk = _probe(rng, keys, n, style)
    pn = rng.random(n) < 0.15
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n, fk,
                            {"fk": pn} if n > 1 else None)
    joins = [join(bt, bd, bn, "bk", "fk", kind="anti",
                  preds=[("v", 200, POS_INF)])]
    aggs = ["count", ("sum", [("x", "id"), ("y", "add100")]),
            ("count", "fk")]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins, [], aggs)
    _check_paths(paths, mode, anti=1)
    assert ("path_plan_join_bitmap" if style == "dense"
            else "path_plan_join_hash") in paths
    if n > 1:
        # every NULL probe key survived; some rows were dropped
        assert exp[0][2][0] - exp[0][2][2] == int(pn.sum()) > 0
        assert exp[0][2][0] < n
        run(eng, mode, t, data, nulls, [("y", 3, 40)], joins, ["g"], aggs)


@pytest.mark.parametrize("style", ["dense", "sparse"])
def test_anti_against_empty_set(eng, mode, style):
    rng = np.random.default_rng(1600)
    n = 257
    tag = f"anti0_{style}_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, 601, style)
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, keys, n, style, present_only=True))
    joins = [join(bt, bd, bn, "bk", "fk", kind="anti",
                  preds=[("v", 5000, POS_INF)])]
    _p, exp, _paths = run(eng, mode, t, data, nulls, [], joins, [],
                          ["count"])
    assert exp == [(0, 0, [n])]


@pytest.mark.parametrize("second", ["inner", "left", "anti", "semi"])
@pytest.mark.parametrize("n", [257, 6001])
def test_chain_through_left_payload(eng, mode, n, second):
    """lineitem LEFT JOIN orders, then orders.ckey against customer: a
    NULL-extended row has a NULL chained key, so INNER and SEMI drop it,
    LEFT NULL-extends it again and ANTI keeps it"""
    rng = np.random.default_rng(1700 + n)
    mo, mc = 601, 3 if n == 257 else 601
    tag = f"ch_{second}_{n}_{mode}"
    ckeys, ct, cd, cn = _build(eng, f"po_c_{tag}", rng, mc, "sparse",
                               unique=second in ("inner", "left"))
    # no INT64_MIN among a SEMI join's probe keys: the SEMI hash-set probe
    # (unchanged here) tests match before empty and takes that key, which
    # encodes as the empty sentinel, for a member
    okeys, ot, od, on = _build(
        eng, f"po_o_{tag}", rng, mo, "dense", {"ckey": rng.random(mo) < 0.1},
        extra=[("ckey", "int64",
                _probe(rng, ckeys, mo,
                       "dense" if second == "semi" else "sparse"))])
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, okeys, n, "dense"))
    joins = [join(ot, od, on, "bk", "fk", kind="left"),
             join(ct, cd, cn, "bk", "ckey", kind=second, probe_src=1)]
    aggs = ["count", ("count", (0, "bk")), ("sum", [((0, "v"), "id")])]
    group = [(0, "c")]
    if second in ("inner", "left"):
        aggs = aggs + [("count", (1, "bk")), ("min", ((1, "w"), "id"))]
        group = [(1, "c")]
    _p, exp, paths = run(eng, mode, t, data, nulls, [], joins, group, aggs)
    _check_paths(paths, mode, left=1 + (second == "left"),
                 anti=second == "anti")
    total = sum(v[0] for _a, _b, v in exp)
    ext0 = total - sum(v[1] for _a, _b, v in exp)
    whole = eval_plan(n, data, nulls, [], joins[:1], [],
                      ["count", ("count", (0, "bk"))])[0][2]
    if second in ("inner", "semi"):
        assert ext0 == 0 and 0 < total < whole[1]
    elif second == "left":
        assert total == n and ext0 == whole[0] - whole[1] > 0
    else:
        assert ext0 == whole[0] - whole[1] > 0 and total < n


def test_left_duplicate_build_keys(eng, mode):
    from greengage_amd import EngineError
    from plan_outer_ref import plan_mode
    rng = np.random.default_rng(1800)
    n, m = 257, 601
    for style in ("dense", "sparse"):
        tag = f"dup_{style}_{mode}"
        ktype, keys = _keys(rng, m, style)
        keys[7] = keys[3]                       # two rows, one key
        v = rng.integers(0, 1000, m).astype(np.int64)
        v[7] = 5000
        kn = np.zeros(m, bool)
        kn[20] = kn[21] = True                  # ... and two NULL keys
        keys[21] = keys[20]
        bt, bd, bn = register(eng, f"po_b_{tag}",
                              [("bk", ktype, keys), ("v", "int64", v)],
                              {"bk": kn})
        t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                                rng.choice(keys.astype(np.int64), n))
        with plan_mode(mode):
            p = eng.compile_plan(t, joins=[{"table": bt, "build_key": "bk",
                                            "probe_key": "fk",
                                            "kind": "left"}],
                                 aggs=["count"])
            with pytest.raises(EngineError, match="status 5:"):
                eng.execute_plan(p, max_groups=8)
        # the duplicate fails the ON-clause, the NULL keys never count
        joins = [join(bt, bd, bn, "bk", "fk", kind="left",
                      preds=[("v", NEG_INF, 5000)])]
        run(eng, mode, t, data, nulls, [], joins, [],
            ["count", ("count", (0, "v"))])


def test_compile_time_rejections(eng):
    from greengage_amd import engine as ge
    rng = np.random.default_rng(1900)
    keys, bt, bd, bn = _build(eng, "po_err_b", rng, 3, "dense")
    t, data, nulls = _drive(eng, "po_err_d", rng, 257,
                            _probe(rng, keys, 257, "dense"))

    def jn(kind, **kw):
        return dict({"table": bt, "build_key": "bk", "probe_key": "fk",
                     "kind": kind}, **kw)

    def status(d):
        h = ctypes.c_int32()
        return ge.lib().gg_engine_compile_plan(ctypes.byref(d),
                                               ctypes.byref(h))

    def desc(kind, **kw):
        return ge.build_plan_desc(t, joins=[jn(kind)], **kw)[0]

    forms = [dict(group_cols=[(0, "c")], aggs=["count"]),
             dict(aggs=[("sum", [((0, "v"), "id")])]),
             dict(aggs=[flt("count", [((0, "w"), 0, 5)])])]
    for kw in forms:
        assert status(desc("anti", **kw)) == EINVAL, kw
        assert status(desc("semi", **kw)) == EINVAL, kw
        assert status(desc("left", **kw)) == 0, kw
        assert status(desc("inner", **kw)) == 0, kw
    # probe_src naming an ANTI join; the same through a LEFT join compiles
    for kind, want in (("anti", EINVAL), ("left", 0)):
        d = ge.build_plan_desc(
            t, joins=[jn(kind), jn("anti", probe_key="s", probe_src=1)],
            aggs=["count"])[0]
        assert status(d) == want, kind
    ge.lib().gg_engine_last_error.restype = ctypes.c_char_p
    assert status(desc("anti", **forms[0])) == EINVAL
    assert b"group_src" in ge.lib().gg_engine_last_error()
    assert status(desc("semi", **forms[0])) == EINVAL
    msg = ge.lib().gg_engine_last_error()
    assert b"group_src" in msg and b"SEMI" in msg
    # kind 4 and -1 are no kinds
    for bad in (4, -1):
        d = desc("anti", aggs=["count"])
        d.joins[0].kind = bad
        assert status(d) == ENOTSUP
    assert status(desc("anti", aggs=["count"])) == 0
    # the engine stays usable
    for mode in ("rtc", "interp"):
        run(eng, mode, t, data, nulls, [],
            [join(bt, bd, bn, "bk", "fk", kind="left")], [], ["count"])


def test_stat_rows_only_where_such_joins_are(eng, mode):
    rng = np.random.default_rng(2000)
    n, m = 257, 601
    tag = f"st_{mode}"
    keys, bt, bd, bn = _build(eng, f"po_b_{tag}", rng, m, "dense")
    t, data, nulls = _drive(eng, f"po_d_{tag}", rng, n,
                            _probe(rng, keys, n, "dense"))
    for kinds in (["semi"], ["inner"], ["semi", "inner"], ["left"],
                  ["anti"], ["anti", "left"], ["left", "left"]):
        joins = [join(bt, bd, bn, "bk", "fk", kind=k) for k in kinds]
        p, _exp, paths = run(eng, mode, t, data, nulls, [], joins, [],
                             ["count"])
        _check_paths(paths, mode, left=kinds.count("left"),
                     anti=kinds.count("anti"))
        by = {s["name"]: s["launches"] for s in eng.stats(p)}
        # one count per such join and execute
        assert by.get("path_plan_join_left", 0) == 3 * kinds.count("left")
        assert by.get("path_plan_join_anti", 0) == 3 * kinds.count("anti")


def test_unchanged_descriptor_still_equals_filter_ref(eng, mode):
    """SEMI + INNER, from plan_filter_gen: what it computed before"""
    import plan_filter_gen as fgen
    import plan_filter_ref as fref
    desc = next(d for d in fgen.all_descs()
                if sorted(j["kind"] for j in d["joins"]) == ["inner", "semi"])
    reg, handles = {}, {}
    for name, (cols, nullmap) in desc["tables"].items():
        h, data, nulls = register(eng, f"po_old_{mode}_{name}", cols, nullmap)
        reg[name], handles[name] = (data, nulls), h
    data, nulls = reg["d"]
    joins = fgen.ref_joins(desc, reg, handles)
    exp = fref.eval_plan(desc["n"], data, nulls, desc["preds"], joins,
                         desc["group"], desc["aggs"])
    _p, _exp, paths = run(eng, mode, handles["d"], data, nulls,
                          desc["preds"], joins, desc["group"], desc["aggs"],
                          exp=exp)
    _check_paths(paths, mode)
