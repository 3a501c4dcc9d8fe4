"""Seeded random descriptors with COUNT(DISTINCT) aggregates, shared by
test_gpu_plan_distinct_fuzz.py (which runs them) and
test_plan_distinct_cpu.py (which checks, without an engine, that the engine
can refuse none of them).

16 descriptors from one fixed seed.  Each is a plan_outer_gen draw (1..2
joins of all four kinds, chains, nullable columns, filters) cut to 0..1 group
columns and 0..3 of its aggregates, with 1..2 DISTINCT aggregates added over
ONE column of any valid source (the driving table or an INNER / LEFT join's
build table), each filtered with probability 1/2; half of the descriptors
get plan_where_gen's WHERE clauses, half an order and a limit.  Every value
column spans far fewer than 2^20 values, so every (group, distinct) pair
fits the 62-bit code: pair_bits restates gg_engine_plan_group_bits' rule.

Everything here is plain numpy (plan_filter_gen.tables_of).
"""
import numpy as np

import plan_outer_gen as outer
import plan_where_gen as wgen
from plan_distinct_ref import eval_plan, pair_count
from plan_filter_gen import MAX_SLOTS, _range, ref_joins, slots, tables_of
from plan_filter_ref import split

SEED = 20261120
NDESC = 16
MAP_KINDS = ("inner", "left")


def _is_avg(a):
    a = split(a)[0]
    return a != "count" and a[0] == "avg"


def _pool(desc):
    """every non-key column of every valid source, with its values"""
    arrays = {}
    for c, _t, a in desc["tables"]["d"][0]:
        if not c.startswith("k"):
            arrays[c] = a
    for j, spec in enumerate(desc["joins"]):
        if spec["kind"] in MAP_KINDS:
            for c, _t, a in desc["tables"][spec["_tname"]][0]:
                if c not in ("bk", "nk"):
                    arrays[(j, c)] = a
    return arrays


def gen(rng, it):
    while True:
        desc = outer._draw(rng, it)
        arrays = _pool(desc)
        cols = list(arrays)
        # the draw's own group columns are tiny; here any column may group,
        # and the wide ones (240 or 10,000 values) are favoured for DISTINCT
        wide = [c for c in cols if (c if isinstance(c, str) else c[1])[-2]
                == "v"]
        desc["group"] = ([] if rng.random() < 0.35 else
                         [cols[int(rng.integers(0, len(cols)))]])
        pick_from = wide if rng.random() < 0.7 else cols
        dcol = pick_from[int(rng.integers(0, len(pick_from)))]
        distinct = []
        for _ in range(int(rng.integers(1, 3))):
            a = ("count_distinct", dcol)
            if rng.random() < 0.5:
                fc = cols[int(rng.integers(0, len(cols)))]
                a = ("filter", a, [(fc,) + _range(rng, arrays[fc])])
            distinct.append(a)
        others = desc["aggs"][:int(rng.integers(0, 4))]
        while slots(dict(desc, aggs=others)) + len(distinct) > MAX_SLOTS:
            others.pop()
        aggs = others + distinct
        order = rng.permutation(len(aggs))
        desc["aggs"] = [aggs[i] for i in order]
        desc["where"] = []
        for spec in desc["joins"]:
            spec["where"] = []
        if rng.random() < 0.5:
            wgen._add_where(rng, desc)
        desc["order_by"], desc["limit"] = [], 0
        if rng.random() < 0.5:
            usable = [i for i, a in enumerate(desc["aggs"]) if not _is_avg(a)]
            for _ in range(int(rng.integers(1, 3))):
                if desc["group"] and rng.random() < 0.3:
                    ent = ("key", 0)
                else:
                    ent = ("agg", usable[int(rng.integers(0, len(usable)))])
                desc["order_by"].append(
                    ent + (["asc", "desc"][int(rng.integers(0, 2))],
                           ["nulls_first", "nulls_last"][
                               int(rng.integers(0, 2))]))
            desc["limit"] = int(rng.choice([0, 1, 3, 5, 50]))
        try:
            from greengage_amd import build_plan_where
            build_plan_where(desc["joins"], desc["where"])
        except ValueError:
            continue
        return desc


def all_descs(seed=SEED):
    rng = np.random.default_rng(seed)
    return [gen(rng, it) for it in range(NDESC)]


def distinct_ref(desc):
    return next(split(a)[0][1] for a in desc["aggs"]
                if split(a)[0] != "count"
                and split(a)[0][0] == "count_distinct")


def _column(desc, c):
    """(type, values) of a column reference, over its whole table"""
    tname = "d" if isinstance(c, str) else desc["joins"][c[0]]["_tname"]
    name = c if isinstance(c, str) else c[1]
    return next((t, a) for n, t, a in desc["tables"][tname][0] if n == name)


def pair_bits(desc):
    """(b0, b1) of the inner plan's packed pair by gg_engine_plan_group_bits'
    rule (bit_length(max - min + 1) over the whole column, values under NULL
    flags included), or None where nothing is packed: no group column, or
    two char1 columns"""
    if not desc["group"]:
        return None
    cols = [_column(desc, desc["group"][0]),
            _column(desc, distinct_ref(desc))]
    if all(t == "char1" for t, _a in cols):
        return None
    return tuple(int(int(a.astype(np.int64).max())
                     - int(a.astype(np.int64).min()) + 1).bit_length()
                 for _t, a in cols)


def expected(desc, reg=None, handles=None, evaluator=eval_plan):
    reg = reg or tables_of(desc)
    data, nulls = reg["d"]
    return evaluator(desc["n"], data, nulls, desc["preds"],
                     ref_joins(desc, reg, handles), desc["group"],
                     desc["aggs"], desc["where"])


def pairs(desc, reg=None, handles=None):
    return expected(desc, reg, handles, pair_count)
