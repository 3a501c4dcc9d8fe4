"""COUNT(DISTINCT) of compiled plans (engine_abi.h GG_AGG_COUNT_DISTINCT),
without a GPU: the constant in the header and the binding, the builder's
spec, the reference (plan_distinct_ref) by hand, and the regroup's shared
functions (greengage_amd/csrc/plan_distinct.h), which the device kernel and
the host path both fold with, compiled from that header alone into a
stand-alone program (plan_distinct_host_main.cpp, its own main) that checks
them against expectations written out by hand.  The program is built twice,
plain and with the address and undefined-behaviour sanitizers, and both
builds are executed directly.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from plan_distinct_ref import NULL_KEY, eval_plan, pair_count

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _header():
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        return f.read()


# ---- constants and the builder ----

def test_constant_matches_header():
    import greengage_amd as g
    from greengage_amd import engine as ge
    src = _header()
    body = re.search(r"typedef enum gg_plan_aggkind\s*\{(.*?)\}\s*"
                     r"gg_plan_aggkind;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    # C's rule: an enumerator without a value takes the previous one's + 1
    kinds, nxt = {}, 0
    for name, val in re.findall(r"GG_AGG_(\w+)\s*(?:=\s*(\d+))?\s*,?", body):
        kinds[name] = nxt = int(val) if val else nxt
        nxt += 1
    assert re.search(r"static_assert\(GG_AGG_COUNT_DISTINCT == 6,", src)
    assert kinds == {"COUNT_STAR": 0, "COUNT_COL": 1, "SUM": 2, "MIN": 3,
                     "MAX": 4, "AVG": 5, "COUNT_DISTINCT": 6}
    assert ge.AGG_COUNT_DISTINCT == g.AGG_COUNT_DISTINCT == 6
    assert (ge.AGG_COUNT_STAR, ge.AGG_COUNT_COL, ge.AGG_SUM, ge.AGG_MIN,
            ge.AGG_MAX, ge.AGG_AVG) == (0, 1, 2, 3, 4, 5)


def test_descriptor_keeps_its_layout():
    import ctypes
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()
    assert [f for f, _t in ge._PlanDesc._fields_][-1] == "est_groups"


def test_builder_spec():
    from greengage_amd import engine as ge
    d, kinds = ge.build_plan_desc(
        0, joins=[{"table": 1, "build_key": "k", "probe_key": "fk",
                   "kind": "left"}],
        group_cols=["g"],
        aggs=[("count_distinct", "x"),
              ("filter", ("count_distinct", (0, "p")), [("y", 0, 5)]),
              "count",
              # passed through for the engine to refuse
              ("count_distinct", [("x", "sub100")]),
              ("count_distinct", [("x", "id"), ("y", "id")])],
        order_by=[("agg", 0, "desc")], limit=3)
    assert kinds == [6, 6, 0, 6, 6]
    a = d.aggs
    assert (a[0].kind, a[0].nfactors, a[0].col[0], a[0].src[0], a[0].mod[0],
            a[0].filter) == (6, 1, b"x", 0, 0, 0)
    assert (a[1].kind, a[1].nfactors, a[1].col[0], a[1].src[0], a[1].mod[0],
            a[1].filter) == (6, 1, b"p", 1, 0, 1)
    assert (a[3].nfactors, a[3].mod[0]) == (1, 1)
    assert (a[4].nfactors, a[4].col[1]) == (2, b"y")
    assert d.nfilters == 1 and d.norder == 1 and d.order[0].index == 0
    # HAVING names it like a COUNT
    h = ge.build_plan_having([("count_distinct", "x")], [("cmp", 0, ">", 2)])
    assert h.nclauses == 1 and h.clauses[0].atoms[0].agg == 0


# ---- the reference by hand ----

def test_reference_by_hand():
    g = np.array([1, 1, 1, 1, 2, 2, 3, 3, 1], np.int64)
    x = np.array([5, 5, 6, 0, 7, 7, 0, 0, 9], np.int64)
    y = np.array([0, 9, 9, 0, 0, 9, 0, 0, 0], np.int64)
    nulls = {"g": np.zeros(9, bool), "x": x == 0, "y": np.zeros(9, bool)}
    nulls["g"][8] = True
    data = {"g": g, "x": x, "y": y}
    aggs = [("count_distinct", "x"), "count", ("count", "x"),
            ("filter", ("count_distinct", "x"), [("y", 0, 1)])]
    # group 1: values {5, 6} and a NULL; under y = 0 only one row with 5
    # group 3: NULL values only; the NULL group: {9}
    assert eval_plan(9, data, nulls, [], [], ["g"], aggs) == [
        (NULL_KEY, 0, [1, 1, 1, 1]), (1, 0, [2, 4, 3, 1]),
        (2, 0, [1, 2, 2, 1]), (3, 0, [0, 2, 0, 0])]
    assert pair_count(9, data, nulls, [], [], ["g"], aggs) == 6
    assert eval_plan(9, data, nulls, [], [], [], aggs) == [
        (0, 0, [4, 9, 6, 3])]
    assert pair_count(9, data, nulls, [], [], [], aggs) == 5
    # no surviving row: the plain aggregate still yields its row
    assert eval_plan(9, data, nulls, [("y", 100, 200)], [], [], aggs) == [
        (0, 0, [0, 0, 0, 0])]
    assert pair_count(9, data, nulls, [("y", 100, 200)], [], [], aggs) == 0
    assert eval_plan(9, data, nulls, [("y", 100, 200)], [], ["g"], aggs) == []


# ---- the shared fold, stand-alone ----

def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(tmp_path, name, extra):
    out = str(tmp_path / name)
    src = os.path.join(HERE, "plan_distinct_host_main.cpp")
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                        src, "-o", out] + extra,
                       capture_output=True, text=True)
    return out, r


def _run(prog):
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stderr == ""
    assert re.fullmatch(r"ok \d+\n", r.stdout), r.stdout
    assert int(r.stdout.split()[1]) >= 40


def test_fold_functions_plain(tmp_path):
    prog, r = _build(tmp_path, "plan_distinct_host", [])
    assert r.returncode == 0, r.stderr
    _run(prog)


def test_fold_functions_sanitized(tmp_path):
    prog, r = _build(tmp_path, "plan_distinct_host_san",
                     ["-fsanitize=address,undefined",
                      "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtimes")
    _run(prog)


# ---- the fuzz generator (test_gpu_plan_distinct_fuzz.py), no engine ----

def test_fuzz_descriptors_cannot_be_refused():
    """every seed's pair fits the packed code by gg_engine_plan_group_bits'
    rule restated in Python (checked against the library's own), its lowered
    form fits the accumulator slots, and the binding builds it"""
    import plan_distinct_gen as gen
    from greengage_amd import engine as ge
    from plan_filter_gen import MAX_SLOTS, slots
    from plan_filter_ref import split
    descs = gen.all_descs()
    assert len(descs) == gen.NDESC == 16
    packed = 0
    for d in descs:
        assert len(d["group"]) <= 1
        kinds = [split(a)[0] if split(a)[0] == "count" else split(a)[0][0]
                 for a in d["aggs"]]
        ndist = kinds.count("count_distinct")
        assert 1 <= ndist <= 2 and len(kinds) - ndist <= 3
        assert len({split(a)[0][1] for a, k in zip(d["aggs"], kinds)
                    if k == "count_distinct"}) == 1
        others = [a for a, k in zip(d["aggs"], kinds)
                  if k != "count_distinct"]
        assert slots(dict(d, aggs=others)) + ndist <= MAX_SLOTS
        for _t, a in (gen._column(d, c) for c in gen._pool(d)):
            assert int(a.max()) - int(a.min()) < 1 << 20
        bits = gen.pair_bits(d)
        if bits is not None:
            packed += 1
            assert max(bits) <= 21 and sum(bits) <= 62
            cols = [gen._column(d, d["group"][0])[1],
                    gen._column(d, gen.distinct_ref(d))[1]]
            st, lib_bits = ge.plan_group_bits(
                [int(c.min()) for c in cols], [int(c.max()) for c in cols])
            assert st == 0 and tuple(lib_bits) == bits
        joins = [dict(j, table=1 + i) for i, j in enumerate(d["joins"])]
        desc, _kinds = ge.build_plan_desc(
            0, d["preds"], joins, d["group"], d["aggs"], d["order_by"],
            d["limit"])
        assert desc.ngroup == len(d["group"])
        ge.build_plan_where(joins, d["where"])
    assert packed >= 6


def test_fuzz_covers_the_ground():
    """what the seed was chosen for, on the reference alone"""
    import plan_distinct_gen as gen
    from plan_filter_ref import split
    descs = gen.all_descs()
    rows = [(d, len(gen.expected(d)), gen.pairs(d)) for d in descs]
    assert sum(bool(d["group"]) for d, _g, _p in rows) >= 8
    assert sum(not d["group"] for d, _g, _p in rows) >= 4
    assert sum(p > 8 for _d, _g, p in rows) >= 10          # device folds
    assert sum(p <= 8 for _d, _g, p in rows) >= 3          # host folds
    assert sum(g > 32 for _d, g, _p in rows) >= 3          # cache overflows
    assert all(g > 0 for _d, g, _p in rows)
    assert sum(not isinstance(gen.distinct_ref(d), str)
               for d, _g, _p in rows) >= 4                 # payload column
    assert sum(bool(d["where"]) for d, _g, _p in rows) >= 4
    assert sum(bool(d["order_by"]) for d, _g, _p in rows) >= 4
    assert sum(any(split(a)[1] is not None and split(a)[0] != "count"
                   and split(a)[0][0] == "count_distinct" for a in d["aggs"])
               for d, _g, _p in rows) >= 4
