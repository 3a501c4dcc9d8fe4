"""Exact reference for compiled plans with LEFT OUTER and ANTI joins
(engine_abi.h gg_plan_joinkind GG_JOIN_LEFT / GG_JOIN_ANTI).

Extends plan_filter_ref's form: a join spec may carry "kind": "left" or
"anti" beside "semi" and "inner", and a column pair (join_index, "col")
may name a LEFT join wherever it may name an INNER one.

Joins run in descriptor order over the rows that passed the WHERE
predicates.  match(j) = the probe key is non-NULL and equals the build key
of some build row that passes join j's build predicates and has a non-NULL
key.  SEMI and INNER drop a row without a match, ANTI drops a row WITH one
(so a NULL probe key survives), LEFT drops nothing.  The two map kinds keep
a per-join array of build-row indices, -1 where the row is NULL-extended
(LEFT without a match) or dead; every payload view has its NULL flag
forced where the index is -1, and the NULL rules of grouping, strict
transitions, filters and chained probe keys then apply by themselves.

With no LEFT and no ANTI join the result is plan_filter_ref.eval_plan's.
"""
import numpy as np

from plan_filter_ref import split
from plan_minmax_ref import _agg
from plan_payload_ref import (NEG_INF, NULL_KEY, POS_INF,  # noqa: F401
                              NotUnique, _vname, join, plan_mode, pred_mask,
                              register, strip)

MAP_KINDS = ("inner", "left")


def _view(spec, col, r):
    """(values, flags) of build column `col` gathered through the index
    array r; -1 reads as NULL"""
    ext = r < 0
    if spec["_n"] == 0:
        return np.zeros(len(r), np.int64), np.ones(len(r), bool)
    rr = np.maximum(r, 0)
    return (np.where(ext, 0, spec["_data"][col][rr]),
            spec["_nulls"][col][rr] | ext)


def resolve_joins(n, data, nulls, preds, joins):
    """(mask of surviving driving rows, [per-join build index or None])"""
    m = pred_mask(preds, data, nulls, n)
    ridx = []
    for j, spec in enumerate(joins):
        bdata, bnulls = spec["_data"], spec["_nulls"]
        bk, pk = spec["build_key"], spec["probe_key"]
        kind = spec.get("kind", "semi")
        assert kind in ("semi", "inner", "left", "anti"), kind
        src = spec.get("probe_src", 0)
        if src == 0:
            pv, pn = data[pk], nulls[pk]
        else:
            assert 1 <= src <= j and ridx[src - 1] is not None, \
                "probe_src must name an earlier INNER or LEFT join"
            pv, pn = _view(joins[src - 1], pk, ridx[src - 1])
        bm = pred_mask(spec.get("preds", ()), bdata, bnulls, spec["_n"])
        bm &= ~bnulls[bk]
        rows = np.nonzero(bm)[0]
        keys = bdata[bk][rows]
        if kind not in MAP_KINDS:
            has = ~pn & np.isin(pv, keys)
            m = m & (has if kind == "semi" else ~has)
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
        if kind == "inner":
            m = hit
    # a row dropped by a later join keeps no partner anywhere
    ridx = [None if r is None else np.where(m, r, -1) for r in ridx]
    return m, ridx


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
                assert ridx[k] is not None, "payload of a SEMI or ANTI join"
                vdata[name], vnulls[name] = _view(joins[k], col, ridx[k])
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


def null_extended(n, data, nulls, preds, joins):
    """per LEFT join: (surviving rows, of which NULL-extended)"""
    m, ridx = resolve_joins(n, data, nulls, preds, joins)
    return {j: (int(m.sum()), int((m & (ridx[j] < 0)).sum()))
            for j, spec in enumerate(joins) if spec.get("kind") == "left"}


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
