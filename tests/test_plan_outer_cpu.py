"""LEFT OUTER and ANTI joins of compiled plans, the parts that need no GPU:
the binding against include/engine_abi.h and the built library, the
reference evaluator (plan_outer_ref) against a row-at-a-time loop and
against plan_filter_ref where no new kind occurs, and the properties the
fuzz seed (plan_outer_gen.SEED) was chosen for."""
import ctypes
import os
import re

import numpy as np

import plan_filter_gen as fgen
import plan_filter_ref as fref
import plan_outer_gen as gen
from plan_outer_ref import NEG_INF, NULL_KEY, POS_INF, eval_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        return f.read()


def test_descriptor_sizes_unchanged():
    """kind was an int all along: neither struct grows"""
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()
    assert ctypes.sizeof(ge._PlanAgg) == 40
    ptr = ctypes.sizeof(ctypes.c_char_p)
    scan = ctypes.sizeof(ge._PlanScan)
    assert ctypes.sizeof(ge._PlanJoin) == scan + 2 * ptr + 8


def test_join_kinds_match_header():
    from greengage_amd import engine as ge
    src = _header()
    body = re.search(r"typedef enum gg_plan_joinkind\s*\{(.*?)\}\s*"
                     r"gg_plan_joinkind;", src, re.S).group(1)
    # the enumerators as C numbers them: an explicit value, else the
    # previous one plus 1
    vals, nxt = {}, 0
    for item in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(","):
        m = re.match(r"\s*(GG_JOIN_\w+)\s*(?:=\s*(\d+))?\s*$", item)
        assert m, item
        nxt = int(m.group(2)) if m.group(2) else nxt
        vals[m.group(1)] = nxt
        nxt += 1
    assert vals == {"GG_JOIN_SEMI": ge.JOIN_SEMI,
                    "GG_JOIN_INNER": ge.JOIN_INNER,
                    "GG_JOIN_LEFT": ge.JOIN_LEFT,
                    "GG_JOIN_ANTI": ge.JOIN_ANTI}
    assert "GG_JOIN_LEFT == 2 && GG_JOIN_ANTI == 3" in src   # static assert
    assert (ge.JOIN_SEMI, ge.JOIN_INNER, ge.JOIN_LEFT, ge.JOIN_ANTI) == \
        (0, 1, 2, 3)
    import greengage_amd
    assert (greengage_amd.JOIN_LEFT, greengage_amd.JOIN_ANTI) == (2, 3)
    for word in ("HJ_FILL_OUTER_TUPLE", "JOIN_ANTI", "nodeHash.c:1070",
                 "JOIN_LASJ_NOTIN"):
        assert word in src, word


def test_builder_join_kinds():
    from greengage_amd import engine as ge
    j = {"table": 4, "build_key": "k", "probe_key": "fk"}
    d, _ = ge.build_plan_desc(3, joins=[j], aggs=["count"])
    assert d.joins[0].kind == 0                 # no kind: SEMI, as ever
    assert ge._PlanDesc().joins[1].kind == 0
    d, _ = ge.build_plan_desc(
        3, joins=[dict(j, kind="left"), dict(j, kind="anti", probe_src=1)],
        group_cols=[(0, "g")], aggs=["count", ("count", (0, "w"))])
    assert [d.joins[k].kind for k in range(2)] == [ge.JOIN_LEFT, ge.JOIN_ANTI]
    assert d.joins[1].probe_src == 1 and d.group_src[0] == 1
    assert d.aggs[1].src[0] == 1


# ---- the evaluator against a row-at-a-time loop ----

def _brute(n, data, nulls, preds, joins, group_cols, aggs):
    """the descriptor semantics one row and one build row at a time, in
    plain Python: no index arrays, no masks"""

    def passes(plist, d, nl, i):
        return all(not nl[c][i] and lo <= d[c][i] < hi for c, lo, hi in plist)

    groups = {}
    for i in range(n):
        if not passes(preds, data, nulls, i):
            continue
        # view[s] = (data, nulls, row), or None = NULL-extended source
        view = {0: (data, nulls, i)}
        alive = True
        for j, J in enumerate(joins):
            src = view[J.get("probe_src", 0)]
            key = None
            if src is not None and not src[1][J["probe_key"]][src[2]]:
                key = int(src[0][J["probe_key"]][src[2]])
            bd, bn = J["_data"], J["_nulls"]
            partners = [] if key is None else [
                b for b in range(J["_n"])
                if passes(J.get("preds", ()), bd, bn, b)
                and not bn[J["build_key"]][b]
                and int(bd[J["build_key"]][b]) == key]
            kind = J.get("kind", "semi")
            if kind in ("inner", "left"):
                assert len(partners) <= 1
            if kind in ("semi", "inner") and not partners:
                alive = False
            if kind == "anti" and partners:
                alive = False
            if not alive:
                break
            if kind in ("inner", "left"):
                view[1 + j] = (bd, bn, partners[0]) if partners else None

        if not alive:
            continue

        def val(c):
            """column value of this row, None = SQL NULL"""
            s, name = (0, c) if isinstance(c, str) else (1 + c[0], c[1])
            v = view[s]
            if v is None or v[1][name][v[2]]:
                return None
            return int(v[0][name][v[2]])

        gk = tuple(NULL_KEY if val(c) is None else val(c) for c in group_cols)
        gk = (gk + (0, 0))[:2]
        acc = groups.setdefault(gk, [[] for _ in aggs])
        for a, spec in enumerate(aggs):
            spec, flt = fref.split(spec)
            if flt is not None and not all(
                    val(c) is not None and lo <= val(c) < hi
                    for c, lo, hi in flt):
                continue
            if spec == "count":
                acc[a].append(1)
                continue
            fs = ([(spec[1], "id")] if spec[0] == "count"
                  else [spec[1]] if spec[0] in ("min", "max") else spec[1])
            xs = [val(c) for c, _m in fs]
            if any(x is None for x in xs):
                continue                        # strict transition
            prod = 1
            for x, (_c, mod) in zip(xs, fs):
                prod *= 100 - x if mod == "sub100" else \
                    100 + x if mod == "add100" else x
            acc[a].append(prod)
    if not group_cols and not groups:
        groups[(0, 0)] = [[] for _ in aggs]
    out = []
    for gk in sorted(groups):
        vals = []
        for spec, v in zip(aggs, groups[gk]):
            spec = fref.split(spec)[0]
            kind = "count" if spec == "count" else spec[0]
            vals.append(len(v) if kind == "count" else sum(v) if kind == "sum"
                        else (sum(v), len(v)) if kind == "avg"
                        else None if not v
                        else min(v) if kind == "min" else max(v))
        out.append((gk[0], gk[1], vals))
    return out


def _tables():
    rng = np.random.default_rng(11)
    n, m = 200, 20

    def table(cols, rows, pnull):
        d = {c: a for c, a in cols.items()}
        nl = {c: rng.random(rows) < pnull for c in d}
        return d, nl

    data, nulls = table({
        "g": rng.integers(0, 3, n), "x": rng.integers(-50, 50, n),
        "k0": rng.integers(-2, 28, n), "k1": rng.integers(0, 26, n),
        "k2": rng.integers(0, 30, n)}, n, 0.1)
    nulls["g"][:] = False
    nulls["g"][::17] = True
    b0, b0n = table({"bk": rng.permutation(np.arange(0, 40))[:m],
                     "w": rng.integers(0, 9, m), "c": rng.integers(0, 3, m),
                     "nk": rng.integers(0, 26, m)}, m, 0.15)
    b1, b1n = table({"bk": rng.integers(0, 24, m),          # duplicates
                     "v": rng.integers(0, 9, m)}, m, 0.15)
    b2, b2n = table({"bk": rng.permutation(np.arange(0, 30))[:m],
                     "z": rng.integers(-9, 9, m)}, m, 0.15)
    return n, data, nulls, (b0, b0n), (b1, b1n), (b2, b2n)


def _join(b, **kw):
    return dict(kw, _data=b[0], _nulls=b[1], _n=len(b[0]["bk"]),
                build_key="bk")


AGGS = ["count", ("count", (0, "w")),
        ("sum", [("x", "id"), ((0, "w"), "add100")]),
        ("min", ((0, "w"), "sub100")), ("max", ("x", "id")),
        ("avg", [((0, "w"), "id")]),
        ("filter", "count", [((0, "w"), 2, 7)]),
        ("filter", ("sum", [("x", "id")]), [((0, "c"), 0, 2), ("x", -30, 30)])]


def test_evaluator_matches_row_loop():
    n, data, nulls, b0, b1, b2 = _tables()
    wh = [("x", -45, 45)]
    on = [("w", 1, POS_INF)]                    # ON-clause of the LEFT join
    cases = {
        "left": ([_join(b0, probe_key="k0", kind="left", preds=on)],
                 [(0, "c")]),
        "left_anti_chain": ([_join(b0, probe_key="k0", kind="left", preds=on),
                             _join(b1, probe_key="nk", kind="anti",
                                   probe_src=1, preds=[("v", 2, POS_INF)])],
                            ["g", (0, "c")]),
        "left_semi_chain": ([_join(b0, probe_key="k0", kind="left"),
                             _join(b1, probe_key="nk", kind="semi",
                                   probe_src=1)], [(0, "c")]),
        "left_inner_chain": ([_join(b0, probe_key="k0", kind="left"),
                              _join(b2, probe_key="nk", kind="inner",
                                    probe_src=1)], [(1, "z"), (0, "c")]),
        "left_left_chain": ([_join(b0, probe_key="k0", kind="left", preds=on),
                             _join(b2, probe_key="nk", kind="left",
                                   probe_src=1)], [(1, "z")]),
        "anti_inner": ([_join(b1, probe_key="k1", kind="anti"),
                        _join(b0, probe_key="k0", kind="inner")], []),
        "semi_left": ([_join(b1, probe_key="k1", kind="semi"),
                       _join(b0, probe_key="k0", kind="left")], ["g"]),
    }
    for name, (joins, group) in cases.items():
        # AGGS read build table b0: join 0, or join 1 behind a SEMI / ANTI
        aggs = AGGS if joins[0]["kind"] in ("left", "inner") \
            else [_retarget(a) for a in AGGS]
        if name == "left_left_chain":
            aggs = aggs + [("count", (1, "z")), ("min", ((1, "z"), "id"))]
        got = eval_plan(n, data, nulls, wh, joins, group, aggs)
        exp = _brute(n, data, nulls, wh, joins, group, aggs)
        assert got == exp, name
        assert sum(v[0] for _a, _b, v in got) > 20, name
    # the LEFT cases really have both sides
    got = eval_plan(n, data, nulls, wh, cases["left"][0], [], AGGS[:2])
    assert 0 < got[0][2][1] < got[0][2][0]
    # a NULL-extended group key lands in the NULL group
    got = eval_plan(n, data, nulls, wh, cases["left"][0], [(0, "c")],
                    ["count"])
    assert got[0][0] == NULL_KEY
    # ANTI keeps NULL probe keys: more rows than SEMI drops
    anti = eval_plan(n, data, nulls, [], [_join(b1, probe_key="k1",
                                                kind="anti")], [], ["count"])
    semi = eval_plan(n, data, nulls, [], [_join(b1, probe_key="k1",
                                                kind="semi")], [], ["count"])
    assert anti[0][2][0] + semi[0][2][0] == n
    assert anti[0][2][0] >= int(nulls["k1"].sum()) > 0


def _retarget(a):
    """the same aggregate with payload sources moved from join 0 to 1"""
    def col(c):
        return c if isinstance(c, str) else (1, c[1])
    a, f = fref.split(a)
    if a != "count":
        if a[0] == "count":
            a = ("count", col(a[1]))
        elif a[0] in ("min", "max"):
            a = (a[0], (col(a[1][0]), a[1][1]))
        else:
            a = (a[0], [(col(c), m) for c, m in a[1]])
    if f is not None:
        a = ("filter", a, [(col(c), lo, hi) for c, lo, hi in f])
    return a


def test_evaluator_equals_filter_ref_without_new_kinds():
    for d in fgen.all_descs():
        assert all(j["kind"] in ("semi", "inner") for j in d["joins"])
        reg = fgen.tables_of(d)
        data, nulls = reg["d"]
        args = (d["n"], data, nulls, d["preds"], fgen.ref_joins(d, reg),
                d["group"], d["aggs"])
        assert eval_plan(*args) == fref.eval_plan(*args), d["it"]


# ---- what the fuzz seed was chosen for ----

def test_fuzz_seed_properties():
    descs = gen.all_descs()
    assert len(descs) == gen.NDESC == 16
    p = gen.properties(descs)
    assert p["left_dense"] >= 4 and p["left_hash"] >= 4, p
    assert p["anti_bitmap"] >= 4 and p["anti_hash"] >= 4, p
    assert p["chained_left"] >= 2 and p["chained_left_anti"] >= 1, p
    assert p["group_left"] >= 3 and p["filter_left"] >= 3, p
    # nothing is refused: accumulator budget, unique INNER / LEFT keys
    assert p["max_slots"] <= gen.MAX_SLOTS
    for d in descs:
        assert 1 <= len(d["joins"]) <= 2 and 1 <= len(d["aggs"]) <= 4
        gen.expected(d)                        # raises NotUnique if not
    assert p["extended"]
    for it, j, live, ext in p["extended"]:
        assert live > 0 and 0.1 * live <= ext <= 0.9 * live, (it, j, live,
                                                              ext)
    assert gen.properties_hold(p)
    assert NEG_INF < 0 < POS_INF
