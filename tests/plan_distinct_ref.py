"""Exact reference for compiled plans with COUNT(DISTINCT) aggregates
(engine_abi.h gg_plan_aggkind), in plan_where_ref's form.

It does not go through the engine's lowering (an inner aggregation by
(group key, value) and a regroup): the surviving rows come from
plan_where_ref.row_masks (preds, joins, WHERE), are grouped by the
descriptor's group columns, and ("count_distinct", c) is the len() of the
Python set of the non-NULL values of c among the group's rows, additionally
masked by the aggregate's filter.  Every other aggregate is
plan_minmax_ref._agg's, as in plan_where_ref.eval_plan.

The result has the other evaluators' shape, sorted (key0, key1, vals), so
plan_having_ref.filter_groups and plan_order_ref.order_groups apply to it.
pair_count gives what the engine's regroup reads: the number of distinct
(group key, value) pairs among the surviving rows, NULLs being values there.
"""
import numpy as np

from plan_filter_ref import split
from plan_minmax_ref import _agg
from plan_outer_ref import _view
from plan_payload_ref import (NEG_INF, NULL_KEY, POS_INF,  # noqa: F401
                              _vname, plan_mode, pred_mask, register, strip)
from plan_where_ref import row_masks


def distinct_col(aggs):
    """the one column the plan's count_distinct aggregates name"""
    cols = {split(a)[0][1] for a in aggs
            if isinstance(split(a)[0], (tuple, list))
            and split(a)[0][0] == "count_distinct"}
    assert len(cols) == 1, cols
    return cols.pop()


def _prepare(n, data, nulls, preds, joins, where):
    _m0, m, ridx = row_masks(n, data, nulls, preds, joins, where)
    # a row the WHERE dropped keeps no partner anywhere
    ridx = [None if r is None else np.where(m, r, -1) for r in ridx]
    vdata, vnulls = {}, {}

    def use(c):
        name = _vname(c)
        if name not in vdata:
            if isinstance(c, str):
                vdata[name], vnulls[name] = data[c], nulls[c]
            else:
                k, colname = c
                assert ridx[k] is not None, "payload of a SEMI or ANTI join"
                vdata[name], vnulls[name] = _view(joins[k], colname, ridx[k])
        return name

    return np.nonzero(m)[0], vdata, vnulls, use


def _group_keys(idx, group_cols, vdata, vnulls, use):
    keys = np.zeros((len(idx), 2), np.int64)
    for g, c in enumerate(group_cols):
        name = use(c)
        keys[:, g] = np.where(vnulls[name][idx], NULL_KEY, vdata[name][idx])
    return keys


def eval_plan(n, data, nulls, preds, joins, group_cols, aggs, where=()):
    idx, vdata, vnulls, use = _prepare(n, data, nulls, preds, joins, where)
    lowered = []
    for a in aggs:
        a, fpreds = split(a)
        if a == "count" or a == ("count",):
            v = "count"
        elif a[0] in ("count", "count_distinct"):
            v = (a[0], use(a[1]))
        elif a[0] in ("min", "max"):
            v = (a[0], (use(a[1][0]), a[1][1]))
        else:
            v = (a[0], [(use(c), mod) for c, mod in a[1]])
        fm = None
        if fpreds is not None:
            fm = pred_mask([(use(c), lo, hi) for c, lo, hi in fpreds],
                           vdata, vnulls, n)
        lowered.append((v, fm))

    def one(v, rows):
        if v != "count" and v[0] == "count_distinct":
            c = v[1]
            return len({int(vdata[c][i]) for i in rows if not vnulls[c][i]})
        return _agg(v, vdata, vnulls, rows)

    def row(rows):
        return [one(v, rows if fm is None else rows[fm[rows]])
                for v, fm in lowered]

    if not group_cols:
        return [(0, 0, row(idx))]
    keys = _group_keys(idx, group_cols, vdata, vnulls, use)
    out = {}
    for k in sorted({(int(a), int(b)) for a, b in keys}):
        out[k] = row(idx[(keys[:, 0] == k[0]) & (keys[:, 1] == k[1])])
    return [(k[0], k[1], v) for k, v in sorted(out.items())]


def pair_count(n, data, nulls, preds, joins, group_cols, aggs, where=()):
    idx, vdata, vnulls, use = _prepare(n, data, nulls, preds, joins, where)
    keys = _group_keys(idx, group_cols, vdata, vnulls, use)
    c = use(distinct_col(aggs))
    return len({(int(k), None if vnulls[c][i] else int(vdata[c][i]))
                for k, i in zip(keys[:, 0], idx)})
