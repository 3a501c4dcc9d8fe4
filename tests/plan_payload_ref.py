"""Exact reference for compiled plans with INNER joins and payload
columns (engine_abi.h gg_plan_join.kind / "column sources").

Extends plan_minmax_ref: a join spec may carry "kind": "inner" and
"probe_src": k, and a group column or aggregate factor may be a pair
(join_index, "col") naming a column of that INNER join's build table.

Joins run in descriptor order.  An INNER join resolves every driving
row to the index of its build row (-1 = no partner) by key lookup among
the build rows that pass the build predicates and have a non-NULL key;
the evaluator itself asserts that those keys are unique.  A NULL probe
key, or one taken from a payload column whose flag is set at the build
row, never matches.  Payload columns are then gathered through those
indices into per-driving-row arrays, flags included, and the grouping
and strict aggregate transitions of plan_minmax_ref run unchanged over
them: a NULL payload group key joins the NULL group, a NULL payload
factor is skipped.

Join specs carry the build table in the evaluator's form under
"_data", "_nulls", "_n" (plan_minmax_ref.register).
"""
import numpy as np

import plan_minmax_ref as base
from plan_minmax_ref import (NEG_INF, NULL_KEY, POS_INF,  # noqa: F401
                             plan_mode, pred_mask, register)


class NotUnique(AssertionError):
    pass


def resolve_joins(n, data, nulls, preds, joins):
    """(mask of surviving driving rows, [per-join build index or None])"""
    m = pred_mask(preds, data, nulls, n)
    ridx = []
    for j, spec in enumerate(joins):
        bdata, bnulls = spec["_data"], spec["_nulls"]
        bk, pk = spec["build_key"], spec["probe_key"]
        src = spec.get("probe_src", 0)
        if src == 0:
            pv, pn = data[pk], nulls[pk]
        else:
            assert 1 <= src <= j and ridx[src - 1] is not None, \
                "probe_src must name an earlier INNER join"
            r = np.maximum(ridx[src - 1], 0)    # dead rows: any index
            sdata, snulls = joins[src - 1]["_data"], joins[src - 1]["_nulls"]
            pv, pn = sdata[pk][r], snulls[pk][r]
        bm = pred_mask(spec.get("preds", ()), bdata, bnulls, spec["_n"])
        bm &= ~bnulls[bk]
        rows = np.nonzero(bm)[0]
        keys = bdata[bk][rows]
        if spec.get("kind", "semi") == "semi":
            m = m & ~pn & np.isin(pv, keys)
            ridx.append(None)
            continue
        if len(np.unique(keys)) != len(keys):
            raise NotUnique(f"join {j}: build key not unique")
        order = np.argsort(keys, kind="stable")
        sk = keys[order]
        if len(sk):
            pos = np.minimum(np.searchsorted(sk, pv), len(sk) - 1)
            hit = m & ~pn & (sk[pos] == pv)
            ridx.append(np.where(hit, rows[order[pos]], -1))
        else:
            hit = np.zeros(n, bool)
            ridx.append(np.full(n, -1, np.int64))
        m = hit
    # a row dropped by a later join keeps no partner anywhere
    ridx = [None if r is None else np.where(m, r, -1) for r in ridx]
    return m, ridx


def _vname(c):
    return c if isinstance(c, str) else f"@{c[0]}.{c[1]}"


def eval_plan(n, data, nulls, preds, joins, group_cols, aggs):
    m, ridx = resolve_joins(n, data, nulls, preds, joins)
    vdata = {"@live": m.astype(np.int64)}
    vnulls = {"@live": np.zeros(n, bool)}

    def use(c):
        name = _vname(c)
        if name in vdata:
            return name
        if isinstance(c, str):
            vdata[name], vnulls[name] = data[c], nulls[c]
        else:
            k, col = c
            assert ridx[k] is not None, "payload of a SEMI join"
            r = np.maximum(ridx[k], 0)
            vdata[name] = joins[k]["_data"][col][r]
            vnulls[name] = joins[k]["_nulls"][col][r]
        return name

    vgroup = [use(c) for c in group_cols]
    vaggs = []
    for a in aggs:
        if a == "count" or a == ("count",):
            vaggs.append("count")
        elif a[0] == "count":
            vaggs.append(("count", use(a[1])))
        elif a[0] in ("min", "max"):
            vaggs.append((a[0], (use(a[1][0]), a[1][1])))
        else:
            vaggs.append((a[0], [(use(c), mod) for c, mod in a[1]]))
    return base.eval_plan(n, vdata, vnulls, [("@live", 1, 2)], [], vgroup,
                          vaggs)


def strip(joins):
    """join specs as Engine.compile_plan takes them"""
    return [{k: v for k, v in j.items() if not k.startswith("_")}
            for j in joins]


def join(table, bdata, bnulls, build_key, probe_key, kind="inner",
         preds=(), probe_src=0):
    return {"table": table, "build_key": build_key, "probe_key": probe_key,
            "kind": kind, "preds": list(preds), "probe_src": probe_src,
            "_data": bdata, "_nulls": bnulls,
            "_n": len(next(iter(bdata.values())))}


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
