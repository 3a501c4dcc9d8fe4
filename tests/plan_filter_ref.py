"""Exact reference for compiled plans with per-aggregate FILTER
predicates (engine_abi.h gg_plan_filter).

Extends plan_payload_ref: an aggregate spec may be wrapped as
("filter", <agg spec>, [(col, lo, hi), ...]), where `col` is a column
name of the driving table or a pair (join_index, "col") naming a column
of that INNER join's build table.

The evaluator does its own grouping, because a filter must not touch it:
the groups come from the rows that survive the WHERE predicates and all
joins, and each aggregate then runs over its group's rows additionally
masked by its own filter (a conjunct over a NULL value is not true; a
payload column's flag is read at the joined build row).  A group none of
whose rows pass a filter is still reported: COUNT 0, SUM 0, MIN/MAX None,
AVG (0, 0).  A plain aggregate yields exactly one row.
"""
import numpy as np

from plan_minmax_ref import _agg
from plan_payload_ref import (NEG_INF, NULL_KEY, POS_INF,  # noqa: F401
                              _vname, join, plan_mode, pred_mask, register,
                              resolve_joins, strip)


def split(spec):
    """(inner aggregate spec, filter predicate list or None)"""
    if isinstance(spec, (tuple, list)) and spec[0] == "filter":
        return spec[1], list(spec[2])
    return spec, None


def eval_plan(n, data, nulls, preds, joins, group_cols, aggs):
    m, ridx = resolve_joins(n, data, nulls, preds, joins)
    vdata, vnulls = {}, {}

    def use(c):
        """per-driving-row view of a column of any source"""
        name = _vname(c)
        if name not in vdata:
            if isinstance(c, str):
                vdata[name], vnulls[name] = data[c], nulls[c]
            else:
                k, col = c
                assert ridx[k] is not None, "payload of a SEMI join"
                r = np.maximum(ridx[k], 0)      # dead rows: any index
                vdata[name] = joins[k]["_data"][col][r]
                vnulls[name] = joins[k]["_nulls"][col][r]
        return name

    lowered = []                # (spec over view names, filter mask or None)
    for a in aggs:
        a, fpreds = split(a)
        if a == "count" or a == ("count",):
            v = "count"
        elif a[0] == "count":
            v = ("count", use(a[1]))
        elif a[0] in ("min", "max"):
            v = (a[0], (use(a[1][0]), a[1][1]))
        else:
            v = (a[0], [(use(c), mod) for c, mod in a[1]])
        fm = None
        if fpreds is not None:
            fm = pred_mask([(use(c), lo, hi) for c, lo, hi in fpreds],
                           vdata, vnulls, n)
        lowered.append((v, fm))

    def row(rows):
        return [_agg(v, vdata, vnulls, rows if fm is None else rows[fm[rows]])
                for v, fm in lowered]

    idx = np.nonzero(m)[0]
    if not group_cols:
        return [(0, 0, row(idx))]
    keys = np.zeros((len(idx), 2), np.int64)
    for g, c in enumerate(group_cols):
        name = use(c)
        keys[:, g] = np.where(vnulls[name][idx], NULL_KEY, vdata[name][idx])
    out = {}
    for k in sorted({(int(a), int(b)) for a, b in keys}):
        rows = idx[(keys[:, 0] == k[0]) & (keys[:, 1] == k[1])]
        out[k] = row(rows)
    return [(k[0], k[1], v) for k, v in sorted(out.items())]


def run(eng, mode, t, data, nulls, preds, joins, group_cols, aggs,
        repeats=3, exp=None):
    """Compile and execute `repeats` times (the baked kernel takes over
    from the second execute where one is made); every execute must equal
    the evaluator bit for bit.  Returns (plan, expected, path stat rows)."""
    n = len(next(iter(data.values())))
    if exp is None:
        exp = eval_plan(n, data, nulls, preds, joins, group_cols, aggs)
    with plan_mode(mode):
        p = eng.compile_plan(t, preds=preds, joins=strip(joins),
                             group_cols=group_cols, aggs=aggs)
        for r in range(repeats):
            got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                         key=lambda g: (g[0], g[1]))
            assert len(got) == len(exp), (r, len(got), len(exp))
            for g, e in zip(got, exp):
                assert (g[0], g[1]) == (e[0], e[1]), (r, g, e)
                assert g[2] == e[2], (r, g, e)
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    return p, exp, paths
