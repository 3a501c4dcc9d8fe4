"""Exact reference for compiled plans with up to four group columns
(engine_abi.h gg_plan_groups).

The joins are resolved by plan_payload_ref.resolve_joins (SEMI and INNER),
or by plan_outer_ref.resolve_joins, which agrees with it on those and adds
LEFT and ANTI, for a plan that holds one of these.  The surviving rows are
then grouped by the TUPLE of their keys, as Python ints: a NULL key, by the
column's own flag or because a LEFT join NULL-extended the row, is NULL_KEY,
separately per column.  The aggregates are plan_minmax_ref's, filters
included (plan_filter_ref.split).

A group is (keys, vals), keys a tuple of G ints: the form of
Engine.execute_plan_keys.  Without an order the groups are sorted by the key
tuple; order_groups and filter_groups are plan_order_ref's and
plan_having_ref's rules over that form.

The packed code itself is modelled too: widths(), the bit widths the engine
derives from whole columns, and code_of(), which packs a key tuple.
"""
import numpy as np

import plan_outer_ref as outer
import plan_payload_ref as payload
from plan_filter_ref import split
from plan_having_ref import passes
from plan_minmax_ref import _agg
from plan_order_ref import nulls_first
from plan_payload_ref import (NULL_KEY, _vname, join, plan_mode,  # noqa: F401
                              pred_mask, register, strip)


def resolve_joins(n, data, nulls, preds, joins):
    if any(j.get("kind", "semi") in ("left", "anti") for j in joins):
        return outer.resolve_joins(n, data, nulls, preds, joins)
    return payload.resolve_joins(n, data, nulls, preds, joins)


def eval_plan(n, data, nulls, preds, joins, group_cols, aggs):
    """[(keys, vals)] sorted by keys"""
    m, ridx = resolve_joins(n, data, nulls, preds, joins)
    vdata, vnulls = {}, {}

    def use(c):
        name = _vname(c)
        if name not in vdata:
            if isinstance(c, str):
                vdata[name], vnulls[name] = data[c], nulls[c]
            else:
                k, col = c
                assert ridx[k] is not None, "payload of a SEMI or ANTI join"
                vdata[name], vnulls[name] = outer._view(joins[k], col, ridx[k])
        return name

    lowered = []
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

    idx = np.nonzero(m)[0]
    cols = []
    for c in group_cols:
        name = use(c)
        cols.append(np.where(vnulls[name][idx], NULL_KEY,
                             vdata[name][idx]).tolist())
    rows_of = {}
    for pos, key in enumerate(zip(*cols)):
        rows_of.setdefault(tuple(int(k) for k in key), []).append(pos)
    out = []
    for key in sorted(rows_of):
        rows = idx[np.asarray(rows_of[key], np.int64)]
        out.append((key, [_agg(v, vdata, vnulls,
                               rows if fm is None else rows[fm[rows]])
                          for v, fm in lowered]))
    return out


def order_groups(groups, order_by=(), limit=0):
    """plan_order_ref.order_groups over (keys, vals) groups: the entries in
    turn, then the key tuple ascending"""
    def key(g):
        out = []
        for ent in order_by:
            what, index, direction = ent[:3]
            if what == "key":
                v = None if g[0][index] == NULL_KEY else g[0][index]
            else:
                v = g[1][index]
                assert not isinstance(v, tuple), "AVG as an order key"
            nf = nulls_first(ent)
            if v is None:
                out.append((0 if nf else 1, 0))
            else:
                out.append((1 if nf else 0, -v if direction == "desc" else v))
        out.append(g[0])
        return tuple(out)
    out = sorted(groups, key=key)
    return out[:limit] if limit > 0 else out


def filter_groups(groups, having):
    return [g for g in groups if passes(having, g[1])]


def column(data_of, c):
    """the whole column a group column reference names; data_of(None) is the
    driving table's data, data_of(k) join k's build table's"""
    return data_of(None)[c] if isinstance(c, str) else data_of(c[0])[c[1]]


def widths(arrays):
    """b_g of each whole column (values under NULL flags included), as
    engine_abi.h states it: bit_length(max - min + 1), 1 for no rows"""
    return [1 if len(a) == 0 else
            (int(np.max(a)) - int(np.min(a)) + 1).bit_length() for a in arrays]


def code_of(keys, mins, bits):
    """the packed code of a key tuple: e_g = 0 for NULL, else v - min + 1;
    field 0 most significant"""
    code = 0
    for k, mn, b in zip(keys, mins, bits):
        e = 0 if k == NULL_KEY else k - mn + 1
        assert 0 <= e < (1 << b), (k, mn, b)
        code = (code << b) | e
    return code


def run(eng, mode, t, data, nulls, preds, joins, group_cols, aggs,
        repeats=3, exp=None, max_groups=1 << 12, **kw):
    """Compile and execute `repeats` times (the baked kernel takes over from
    the second execute where one is made); every execute must equal `exp`
    (default: the evaluator's unordered result) bit for bit and in order.
    kw goes to compile_plan (order_by, limit, having, est_groups).  Returns
    (plan, expected, path stat rows)."""
    n = len(next(iter(data.values())))
    if exp is None:
        exp = eval_plan(n, data, nulls, preds, joins, group_cols, aggs)
    with plan_mode(mode):
        p = eng.compile_plan(t, preds=preds, joins=strip(joins),
                             group_cols=group_cols, aggs=aggs, **kw)
        for r in range(repeats):
            got = eng.execute_plan_keys(p, max_groups=max_groups)
            assert len(got) == len(exp), (r, len(got), len(exp))
            for g, e in zip(got, exp):
                assert tuple(g[0]) == tuple(e[0]), (r, g, e)
                assert g[1] == e[1], (r, g, e)
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    return p, exp, paths
