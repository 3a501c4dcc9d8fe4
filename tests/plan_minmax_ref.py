"""Exact reference for compiled plans with MIN/MAX/AVG aggregates.

A restatement of the descriptor semantics (engine_abi.h gg_plan_desc)
shared by the MIN/MAX/AVG plan tests and their multi-process worker:
conjunctive half-open range predicates (NULL fails the qual), hash
SEMI-joins (NULL keys never match), group by 0..2 columns (NULL keys
group together as NULL_KEY), strict aggregate transitions.  Sums are
exact Python ints; MIN/MAX are numpy int64 min/max over the non-NULL
rows of each group.

`data[col]` is an int64 numpy array of the column's values (char1 as
0..255), `nulls[col]` a bool array.  The result has the shape
Engine.execute_plan returns: sorted (key0, key1, vals), one vals entry
per descriptor aggregate — int for COUNT/SUM, int or None for MIN/MAX,
(sum, count) for AVG.
"""
import contextlib
import os

import numpy as np

NULL_KEY = -(1 << 63) + 1
NEG_INF = -(1 << 63)
POS_INF = (1 << 63) - 1


def pred_mask(preds, data, nulls, n):
    m = np.ones(n, bool)
    for cname, lo, hi in preds:
        v = data[cname]
        m &= ~nulls[cname] & (v >= lo) & (v < hi)
    return m


def _factor(data, c, mod, rows):
    x = data[c][rows]
    if mod == "sub100":
        return 100 - x
    if mod == "add100":
        return 100 + x
    return x


def _exact_sum(factors):
    """sum of the elementwise product of int64 arrays, as a Python int"""
    if not len(factors[0]):
        return 0
    bound = len(factors[0])
    for f in factors:
        bound *= max(1, abs(int(f.min())), abs(int(f.max())))
    if bound < (1 << 62):
        v = factors[0].copy()
        for f in factors[1:]:
            v *= f
        return int(v.sum())
    v = factors[0].astype(object)
    for f in factors[1:]:
        v = v * f.astype(object)
    return sum(v.tolist())


def _agg(spec, data, nulls, rows):
    if spec == "count":
        return len(rows)
    if spec[0] == "count":
        return int(np.count_nonzero(~nulls[spec[1]][rows]))
    if spec[0] in ("min", "max"):
        c, mod = spec[1]
        r = rows[~nulls[c][rows]]
        if not len(r):
            return None
        x = _factor(data, c, mod, r)
        return int(x.min() if spec[0] == "min" else x.max())
    ok = np.ones(len(rows), bool)
    for c, _m in spec[1]:
        ok &= ~nulls[c][rows]
    r = rows[ok]
    s = _exact_sum([_factor(data, c, m, r) for c, m in spec[1]])
    return s if spec[0] == "sum" else (s, len(r))


def eval_plan(n, data, nulls, preds, joins, group_cols, aggs):
    m = pred_mask(preds, data, nulls, n)
    for j in joins:
        bdata, bnulls = j["_data"], j["_nulls"]
        bm = pred_mask(j.get("preds", ()), bdata, bnulls, j["_n"])
        bk, pk = j["build_key"], j["probe_key"]
        keys = bdata[bk][bm & ~bnulls[bk]]
        m &= ~nulls[pk] & np.isin(data[pk], keys)
    idx = np.nonzero(m)[0]
    if not group_cols:
        # plain aggregate: exactly one row, even over zero input rows
        return [(0, 0, [_agg(a, data, nulls, idx) for a in aggs])]
    keys = np.zeros((len(idx), 2), np.int64)
    for g, c in enumerate(group_cols):
        keys[:, g] = np.where(nulls[c][idx], NULL_KEY, data[c][idx])
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    bounds = np.searchsorted(inv[order], np.arange(len(uniq) + 1))
    out = []
    for g in range(len(uniq)):
        rows = idx[order[bounds[g]:bounds[g + 1]]]
        out.append((int(uniq[g, 0]), int(uniq[g, 1]),
                    [_agg(a, data, nulls, rows) for a in aggs]))
    return sorted(out, key=lambda r: (r[0], r[1]))


def register(eng, name, cols, nullmap=None):
    """cols: [(name, type, array)]; nullmap: {name: bool/uint8 array}.
    Returns (handle, data, nulls) in the evaluator's form."""
    n = len(cols[0][2])
    t = eng.register_table(name, cols, n)
    data = {c: np.asarray(a).astype(np.int64) for c, _ty, a in cols}
    nulls = {c: np.zeros(n, bool) for c, _ty, _a in cols}
    for c, nl in (nullmap or {}).items():
        eng.set_nulls(t, c, np.asarray(nl).astype(np.uint8))
        nulls[c] = np.asarray(nl).astype(bool)
    return t, data, nulls


def canon(groups):
    """execute_plan output in comparable form (AVG tuples -> lists
    survive a JSON round trip the same way)."""
    return [[k0, k1, [list(v) if isinstance(v, tuple) else v
                      for v in vals]] for k0, k1, vals in groups]


@contextlib.contextmanager
def plan_mode(mode):
    """GG_PLAN_RTC=0 routes a plan to the interpreted kernel; the
    choice is made at the plan's first execute."""
    if mode == "interp":
        os.environ["GG_PLAN_RTC"] = "0"
    try:
        yield
    finally:
        os.environ.pop("GG_PLAN_RTC", None)


def run(eng, mode, t, data, nulls, preds, group_cols, aggs, repeats=1,
        exp=None):
    n = len(next(iter(data.values())))
    if exp is None:
        exp = eval_plan(n, data, nulls, preds, [], group_cols, aggs)
    with plan_mode(mode):
        p = eng.compile_plan(t, preds=preds, group_cols=group_cols,
                             aggs=aggs)
        for r in range(repeats):
            got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                         key=lambda g: (g[0], g[1]))
            assert len(got) == len(exp), (r, len(got), len(exp))
            for g, e in zip(got, exp):
                assert (g[0], g[1]) == (e[0], e[1]), (r, g, e)
                assert g[2] == e[2], (r, g, e)
    return p, exp
