"""Exact reference for compiled plans with general WHERE clauses
(engine_abi.h gg_plan_where): OR / IN / NOT, column-against-column
comparisons and IS [NOT] NULL, for the plan's WHERE and for the build
filter of each join.

Extends plan_outer_ref's form: eval_plan takes `where`, a list of clauses
(ANDed) in Engine.compile_plan's syntax, and a join spec may carry "where",
the clauses of that join's build filter over the build table's own columns.
A clause is a list of atoms (ORed) or one atom:

  ("range", col, lo, hi) | ("not_range", col, lo, hi)
  ("eq", col, v) | ("ne", col, v) | ("in", col, [v...])
  ("cmp", a, op, b)  with op in < <= = <> > >=
  ("is_null", col) | ("not_null", col)
  and the whole clause ("not_in", col, [v...])

Two evaluators.  `eval_plan` is vectorised and two-valued, the way the
engine states the rule: an atom is true or not true, a comparison over a
NULL is not true, a clause is true iff some atom is, a row survives iff
every clause is true.  `naive_plan` shares no code with it: it walks the
rows one by one with Python None as SQL NULL and literal Kleene AND / OR /
NOT over the clauses AS WRITTEN (a "not_in" is NOT (a = v1 OR ...), a "ne"
is NOT (a = v)), and keeps the row iff the qual is True.  It exists to
check the first.

With no clause anywhere the result is plan_outer_ref.eval_plan's.
"""
import numpy as np

from plan_filter_ref import split
from plan_minmax_ref import _agg
from plan_outer_ref import MAP_KINDS, _view
from plan_payload_ref import (NEG_INF, NULL_KEY, POS_INF,  # noqa: F401
                              NotUnique, _vname, join, plan_mode, pred_mask,
                              register, strip)

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
_OPS = {"<": np.less, "<=": np.less_equal, "=": np.equal,
        "<>": np.not_equal, ">": np.greater, ">=": np.greater_equal}


def _is_atom(c):
    return isinstance(c, tuple) and len(c) > 0 and isinstance(c[0], str)


def clauses_of(where):
    """`where` as a list of clauses, each a list of atoms; a "not_in"
    clause becomes one clause per value"""
    out = []
    for cl in where:
        if _is_atom(cl) and cl[0] == "not_in":
            out += [[("ne", cl[1], v)] for v in cl[2]]
        elif _is_atom(cl):
            out.append([cl])
        else:
            out.append(list(cl))
    return out


def atom_mask(a, col):
    """bool array: the atom is TRUE.  col(c) -> (int64 values, NULL flags)"""
    tag = a[0]
    v, nl = col(a[1])
    if tag == "is_null":
        return nl.copy()
    if tag == "not_null":
        return ~nl
    if tag == "range":
        return ~nl & (v >= a[2]) & (v < a[3])
    if tag == "not_range":
        return ~nl & ((v < a[2]) | (v >= a[3]))
    if tag == "eq":
        return ~nl & (v == a[2])
    if tag == "ne":
        return ~nl & (v != a[2])
    if tag == "in":
        return ~nl & np.isin(v, np.asarray(list(a[2]), np.int64))
    assert tag == "cmp", a
    w, wl = col(a[3])
    return ~nl & ~wl & _OPS[a[2]](v, w)


def where_mask(where, col, n):
    m = np.ones(n, bool)
    for cl in clauses_of(where):
        t = np.zeros(n, bool)
        for a in cl:
            t |= atom_mask(a, col)
        m &= t
    return m


def build_mask(spec):
    """build rows of a join that can be partners: the build preds, the
    join's "where" clauses, and a non-NULL key"""
    bdata, bnulls = spec["_data"], spec["_nulls"]
    bm = pred_mask(spec.get("preds", ()), bdata, bnulls, spec["_n"])
    bm &= where_mask(spec.get("where", ()),
                     lambda c: (bdata[c], bnulls[c]), spec["_n"])
    return bm & ~bnulls[spec["build_key"]]


def resolve_joins(n, data, nulls, preds, joins):
    """plan_outer_ref.resolve_joins with build_mask for the build side"""
    m = pred_mask(preds, data, nulls, n)
    ridx = []
    for j, spec in enumerate(joins):
        bk, pk = spec["build_key"], spec["probe_key"]
        kind = spec.get("kind", "semi")
        src = spec.get("probe_src", 0)
        if src == 0:
            pv, pn = data[pk], nulls[pk]
        else:
            pv, pn = _view(joins[src - 1], pk, ridx[src - 1])
        rows = np.nonzero(build_mask(spec))[0]
        keys = spec["_data"][bk][rows]
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
    ridx = [None if r is None else np.where(m, r, -1) for r in ridx]
    return m, ridx


def row_masks(n, data, nulls, preds, joins, where=()):
    """(rows that preds and joins keep, of which the WHERE keeps, ridx)"""
    m, ridx = resolve_joins(n, data, nulls, preds, joins)

    def col(c):
        if isinstance(c, str):
            return data[c], nulls[c]
        return _view(joins[c[0]], c[1], ridx[c[0]])

    return m, m & where_mask(where, col, n), ridx


def eval_plan(n, data, nulls, preds, joins, group_cols, aggs, where=()):
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
        out[k] = row(idx[(keys[:, 0] == k[0]) & (keys[:, 1] == k[1])])
    return [(k[0], k[1], v) for k, v in sorted(out.items())]


# ---- the naive evaluator: None is SQL NULL, Kleene logic, row by row ----

def k_not(x):
    return None if x is None else not x


def k_or(xs):
    xs = list(xs)
    if any(x is True for x in xs):
        return True
    return None if any(x is None for x in xs) else False


def k_and(xs):
    xs = list(xs)
    if any(x is False for x in xs):
        return False
    return None if any(x is None for x in xs) else True


def _k_cmp(op, a, b):
    if a is None or b is None:
        return None
    return {"<": a < b, "<=": a <= b, "=": a == b, "<>": a != b,
            ">": a > b, ">=": a >= b}[op]


def k_atom(a, val):
    """Kleene value of an atom AS WRITTEN; val(c) -> int or None"""
    tag = a[0]
    if tag == "is_null":
        return val(a[1]) is None
    if tag == "not_null":
        return k_not(val(a[1]) is None)
    if tag == "range":
        x = val(a[1])
        return k_and([_k_cmp(">=", x, a[2]), _k_cmp("<", x, a[3])])
    if tag == "not_range":
        return k_not(k_atom(("range",) + tuple(a[1:]), val))
    if tag == "eq":
        return _k_cmp("=", val(a[1]), a[2])
    if tag == "ne":
        return k_not(_k_cmp("=", val(a[1]), a[2]))
    if tag == "in":
        x = val(a[1])
        return k_or(_k_cmp("=", x, v) for v in a[2])
    if tag == "not_in":
        return k_not(k_atom(("in", a[1], a[2]), val))
    assert tag == "cmp", a
    return _k_cmp(a[2], val(a[1]), val(a[3]))


def k_qual(where, val):
    """the qual keeps the row iff it is True (ExecQual)"""
    return k_and(k_atom(cl, val) if _is_atom(cl)
                 else k_or(k_atom(a, val) for a in cl)
                 for cl in where) is True


def naive_plan(n, data, nulls, preds, joins, group_cols, aggs, where=()):
    def cell(d, nl, c, i):
        return None if nl[c][i] else int(d[c][i])

    def rng_ok(plist, val):
        return k_and(k_and([_k_cmp(">=", val(c), lo), _k_cmp("<", val(c), hi)])
                     for c, lo, hi in plist) is True

    maps = []
    for j, spec in enumerate(joins):
        bd, bn = spec["_data"], spec["_nulls"]
        mp = {}
        for r in range(spec["_n"]):
            def bval(c, r=r):
                return cell(bd, bn, c, r)
            if not rng_ok(spec.get("preds", ()), bval):
                continue
            if not k_qual(spec.get("where", ()), bval):
                continue
            k = bval(spec["build_key"])
            if k is None:
                continue
            if k in mp and spec.get("kind", "semi") in MAP_KINDS:
                raise NotUnique(f"join {j}")
            mp[k] = r
        maps.append(mp)

    groups = {}
    for i in range(n):
        part = {}               # join -> build row or None (NULL-extended)

        def val(c, i=i, part=part):
            if isinstance(c, str):
                return cell(data, nulls, c, i)
            r = part[c[0]]
            if r is None:
                return None
            return cell(joins[c[0]]["_data"], joins[c[0]]["_nulls"], c[1], r)

        if not rng_ok(preds, val):
            continue
        alive = True
        for j, spec in enumerate(joins):
            src = spec.get("probe_src", 0)
            pk = val(spec["probe_key"] if src == 0
                     else (src - 1, spec["probe_key"]))
            r = None if pk is None else maps[j].get(pk)
            kind = spec.get("kind", "semi")
            if kind == "left":
                part[j] = r
            elif kind == "anti":
                alive = r is None
            else:
                alive = r is not None
                part[j] = r
            if not alive:
                break
        if not alive or not k_qual(where, val):
            continue
        key = tuple(NULL_KEY if val(c) is None else val(c)
                    for c in group_cols) + (0,) * (2 - len(group_cols))
        groups.setdefault(key, []).append(val)
    if not group_cols:
        groups.setdefault((0, 0), [])

    def agg(a, vals):
        a, fpreds = split(a)
        if fpreds is not None:
            vals = [v for v in vals if rng_ok(fpreds, v)]
        if a == "count" or a == ("count",):
            return len(vals)
        if a[0] == "count":
            return sum(v(a[1]) is not None for v in vals)

        def fac(v, c, mod):
            x = v(c)
            if x is None:
                return None
            return 100 - x if mod == "sub100" else 100 + x if mod == "add100" \
                else x

        if a[0] in ("min", "max"):
            xs = [fac(v, *a[1]) for v in vals]
            xs = [x for x in xs if x is not None]
            return None if not xs else (min(xs) if a[0] == "min" else max(xs))
        s, cnt = 0, 0
        for v in vals:
            fs = [fac(v, c, m) for c, m in a[1]]
            if any(f is None for f in fs):
                continue
            p = 1
            for f in fs:
                p *= f
            s += p
            cnt += 1
        return s if a[0] == "sum" else (s, cnt)

    return [(k[0], k[1], [agg(a, vals) for a in aggs])
            for k, vals in sorted(groups.items())]


def run(eng, mode, t, data, nulls, preds, joins, group_cols, aggs, where=(),
        repeats=3, exp=None, **kw):
    """Compile and execute `repeats` times (the baked kernel takes over
    from the second execute where one is made); every execute must equal
    the evaluator bit for bit.  Returns (plan, expected, path stat rows)."""
    n = len(next(iter(data.values())))
    if exp is None:
        exp = eval_plan(n, data, nulls, preds, joins, group_cols, aggs, where)
    with plan_mode(mode):
        p = eng.compile_plan(t, preds=preds, joins=strip(joins),
                             group_cols=group_cols, aggs=aggs, where=where,
                             **kw)
        for r in range(repeats):
            got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                         key=lambda g: (g[0], g[1]))
            assert len(got) == len(exp), (r, len(got), len(exp))
            for g, e in zip(got, exp):
                assert (g[0], g[1]) == (e[0], e[1]), (r, g, e)
                assert g[2] == e[2], (r, g, e)
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    return p, exp, paths
