"""ctypes bindings for the C-ABI engine (include/engine_abi.h).

The engine library is product native code (HIP gfx950 + RCCL); this
module is plumbing only.  It fails loudly if the library is missing —
no silent CPU fallback (project rule: GPU tests must run the native
path).
"""
import ctypes
import datetime
import os
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_DIR, "libgreengage_engine.so")

I8 = ctypes.c_uint8
I32 = ctypes.c_int32
I64 = ctypes.c_int64
U64 = ctypes.c_uint64


class EngineError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("n_segments", ctypes.c_int),
                ("segment_id", ctypes.c_int), ("hbm_limit_bytes", U64)]


class _ColumnDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("type", ctypes.c_int),
                ("host_data", ctypes.c_void_p),
                ("device_data", ctypes.c_void_p)]


class _PipelineDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("lineitem", I32), ("orders", I32),
                ("customer", I32), ("supplier", I32), ("nation", I32),
                ("cutoff_date", I32), ("cutoff_hi", I32), ("mktsegment", I8),
                ("regionkey", I8), ("limit_k", I64)]


class _PlanPred(ctypes.Structure):
    _fields_ = [("col", ctypes.c_char_p), ("lo", I64), ("hi", I64)]


class _PlanScan(ctypes.Structure):
    _fields_ = [("table", I32), ("preds", _PlanPred * 8),
                ("npreds", ctypes.c_int)]


class _PlanJoin(ctypes.Structure):
    _fields_ = [("build", _PlanScan), ("build_key", ctypes.c_char_p),
                ("probe_key", ctypes.c_char_p), ("kind", ctypes.c_int),
                ("probe_src", ctypes.c_int8)]


class _PlanAgg(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("nfactors", ctypes.c_int),
                ("col", ctypes.c_char_p * 3), ("mod", ctypes.c_int8 * 3),
                ("src", ctypes.c_int8 * 3), ("filter", ctypes.c_int8)]


PLAN_MAX_FILTERS = 4          # GG_PLAN_MAX_FILTERS
PLAN_MAX_FILTER_PREDS = 4     # GG_PLAN_MAX_FILTER_PREDS


class _PlanFilter(ctypes.Structure):
    _fields_ = [("preds", _PlanPred * PLAN_MAX_FILTER_PREDS),
                ("src", ctypes.c_int8 * PLAN_MAX_FILTER_PREDS),
                ("npreds", ctypes.c_int)]


PLAN_MAX_ORDER = 4            # GG_PLAN_MAX_ORDER
PLAN_MAX_LIMIT = 1024         # GG_PLAN_MAX_LIMIT (device top-k)


class _PlanOrder(ctypes.Structure):
    _fields_ = [("what", ctypes.c_int8), ("index", ctypes.c_int8),
                ("desc", ctypes.c_int8), ("nulls_first", ctypes.c_int8)]


class _PlanDesc(ctypes.Structure):
    _fields_ = [("scan", _PlanScan), ("joins", _PlanJoin * 2),
                ("njoins", ctypes.c_int),
                ("group_cols", ctypes.c_char_p * 2),
                ("ngroup", ctypes.c_int), ("aggs", _PlanAgg * 8),
                ("naggs", ctypes.c_int), ("group_src", ctypes.c_int8 * 2),
                ("filters", _PlanFilter * PLAN_MAX_FILTERS),
                ("nfilters", ctypes.c_int),
                ("order", _PlanOrder * PLAN_MAX_ORDER),
                ("norder", ctypes.c_int), ("limit", I64),
                ("est_groups", I64)]


PLAN_MAX_CLAUSES = 8          # GG_PLAN_MAX_CLAUSES
PLAN_MAX_ATOMS = 8            # GG_PLAN_MAX_ATOMS
PLAN_MAX_WHERE_ATOMS = 16     # GG_PLAN_MAX_WHERE_ATOMS
# gg_plan_atomkind (engine_abi.h)
ATOM_RANGE, ATOM_NOT_RANGE = 0, 1
ATOM_LT, ATOM_LE, ATOM_EQ, ATOM_NE = 2, 3, 4, 5
ATOM_IS_NULL, ATOM_NOT_NULL = 6, 7


class _PlanAtom(ctypes.Structure):
    _fields_ = [("col", ctypes.c_char_p), ("col2", ctypes.c_char_p),
                ("lo", I64), ("hi", I64), ("kind", ctypes.c_int8),
                ("src", ctypes.c_int8), ("src2", ctypes.c_int8)]


class _PlanClause(ctypes.Structure):
    _fields_ = [("atoms", _PlanAtom * PLAN_MAX_ATOMS),
                ("natoms", ctypes.c_int), ("scope", ctypes.c_int8)]


class _PlanWhere(ctypes.Structure):
    _fields_ = [("clauses", _PlanClause * PLAN_MAX_CLAUSES),
                ("nclauses", ctypes.c_int)]


PLAN_MAX_HAVING_CLAUSES = 4   # GG_PLAN_MAX_HAVING_CLAUSES
PLAN_MAX_HAVING_ATOMS = 4     # GG_PLAN_MAX_HAVING_ATOMS
PLAN_MAX_HAVING_TOTAL = 8     # GG_PLAN_MAX_HAVING_TOTAL
# gg_plan_havingkind (engine_abi.h)
HAVING_RANGE, HAVING_NOT_RANGE = 0, 1
HAVING_IS_NULL, HAVING_NOT_NULL = 2, 3
# signed 128-bit bounds of a HAVING atom; as lo / hi they mean "no test"
HAVING_NEG_INF = -(1 << 127)
HAVING_POS_INF = (1 << 127) - 1


class _PlanHavingAtom(ctypes.Structure):
    _fields_ = [("lo_lo", U64), ("lo_hi", I64), ("hi_lo", U64),
                ("hi_hi", I64), ("kind", ctypes.c_int8),
                ("agg", ctypes.c_int8)]


class _PlanHavingClause(ctypes.Structure):
    _fields_ = [("atoms", _PlanHavingAtom * PLAN_MAX_HAVING_ATOMS),
                ("natoms", ctypes.c_int)]


class _PlanHaving(ctypes.Structure):
    _fields_ = [("clauses", _PlanHavingClause * PLAN_MAX_HAVING_CLAUSES),
                ("nclauses", ctypes.c_int)]


NEG_INF = -(1 << 63)          # one-sided range bounds
POS_INF = (1 << 63) - 1
PLAN_NULL_KEY = -(1 << 63) + 1
# gg_plan_aggkind (engine_abi.h)
AGG_COUNT_STAR, AGG_COUNT_COL, AGG_SUM = 0, 1, 2
AGG_MIN, AGG_MAX, AGG_AVG = 3, 4, 5
AGG_COUNT_DISTINCT = 6
# gg_plan_joinkind (engine_abi.h)
JOIN_SEMI, JOIN_INNER = 0, 1
JOIN_LEFT, JOIN_ANTI = 2, 3


def build_plan_desc(scan_table, preds=(), joins=(), group_cols=(),
                    aggs=(), order_by=(), limit=0, est_groups=0):
    """The gg_plan_desc (engine_abi.h) of a compositional plan and the
    aggregate kinds execute_plan decodes by: (desc, kinds).  Pure: calls
    neither the library nor a GPU.

    preds: [(col, lo, hi)]  (half-open; NEG_INF/POS_INF one-sided)
    joins: [{"table": h, "build_key": c, "probe_key": c,
             "preds": [...], "kind": "semi"|"inner"|"left"|"anti",
             "probe_src": k}]
           "semi" (default) is a filter; "inner" joins a
           unique-keyed build table whose columns the plan can then
           read.  "left" is "inner" that keeps a row without a
           partner: every column of that build table then reads as
           NULL for it (NULL group, skipped factor, filter not
           true, chained probe key matches nothing), and "preds"
           are ON-clause conditions that never drop a driving row.
           "anti" is NOT EXISTS: the row survives iff it has no
           partner; a NULL probe key survives.  probe_src k takes
           probe_key from the build table of the earlier INNER or
           LEFT join k-1 (0 = driving table).
    group_cols: 0-4 columns of any accepted type (char1, int32,
           int64) and source.  Two char1 columns keep their fixed
           code; any other pair, and every list of three or four,
           is packed into one 64-bit code by the columns' value
           ranges and must fit 62 bits (plan_group_bits,
           plan_group_bits_n).  The ranges are resolved at the first
           execute, which raises EngineError status 5 for columns
           that do not fit.  The descriptor holds the first two
           columns; build_plan_groups holds the others.
    aggs: ["count"] | ("count", col) | ("count_distinct", col) |
          ("sum", [(col, "id"|"sub100"|"add100"), ...]) |
          ("min", (col, mod)) | ("max", (col, mod)) |
          ("avg", [(col, mod), ...]) |
          ("filter", <any of the above>, [(col, lo, hi), ...])
          The last form is agg(...) FILTER (WHERE ...): the aggregate
          sees only the surviving rows on which every half-open range
          holds (a NULL value fails it).  Groups are unaffected; a group
          with no passing row reports COUNT 0, SUM 0, MIN/MAX None,
          AVG (0, 0), COUNT(DISTINCT) 0.  ("count_distinct", col) counts
          the distinct non-NULL values of one column per group; with a
          filter, a value counts if some row carrying it passes.  It goes
          with at most one group column, and every count_distinct of a
          plan names the same column (the engine refuses the rest with
          status 5); est_groups then estimates the distinct (group key,
          value) pairs.  Equal predicate lists share one entry of the
          descriptor's filters[]; more than PLAN_MAX_FILTERS distinct
          lists, or more than PLAN_MAX_FILTER_PREDS ranges in one, raise
          ValueError.
    order_by: up to PLAN_MAX_ORDER entries
          ("agg", a, "asc"|"desc"[, "nulls_first"|"nulls_last"]) |
          ("key", g, "asc"|"desc"[, "nulls_first"|"nulls_last"])
          ordering the groups by descriptor aggregate a (COUNT, SUM, MIN
          or MAX; not AVG) or group column g.  Where the NULL placement
          is omitted, PostgreSQL's default is filled in: NULLS LAST for
          "asc", NULLS FIRST for "desc" (the ABI itself has no default).
          Ties fall back to (key0, key1) ascending, so the order is
          total.  Empty = the (key0, key1) order.
    limit: 0 = every group; > 0 = at most that many, the first of the
          order (up to PLAN_MAX_LIMIT they are selected on the device).
    est_groups: 0 = the fixed group table; > 0 = an estimate of the
          number of groups, which sizes the table and lets it grow.
    The defaults leave the descriptor's tail zero.
    A group column, aggregate factor or filter `col` is a column name of
    the driving table, or a pair (join_index, name) for a column of
    that INNER or LEFT join's build table.
    """
    mods = {"id": 0, "sub100": 1, "add100": 2}
    jkinds = {"semi": JOIN_SEMI, "inner": JOIN_INNER, "left": JOIN_LEFT,
              "anti": JOIN_ANTI}

    def colref(c):
        """(name bytes, source): 0 = driving, 1+k = join k"""
        if isinstance(c, str):
            return c.encode(), 0
        k, name = c
        return name.encode(), 1 + k

    def fill_scan(dst, table, plist):
        dst.table = table
        dst.npreds = len(plist)
        for i, (c, lo, hi) in enumerate(plist):
            dst.preds[i].col = c.encode()
            dst.preds[i].lo = lo
            dst.preds[i].hi = hi

    d = _PlanDesc()
    fill_scan(d.scan, scan_table, list(preds))
    d.njoins = len(joins)
    for j, spec in enumerate(joins):
        fill_scan(d.joins[j].build, spec["table"],
                  list(spec.get("preds", ())))
        d.joins[j].build_key = spec["build_key"].encode()
        d.joins[j].probe_key = spec["probe_key"].encode()
        d.joins[j].kind = jkinds[spec.get("kind", "semi")]
        d.joins[j].probe_src = spec.get("probe_src", 0)
    # columns 2 and 3 travel beside the descriptor (build_plan_groups)
    d.ngroup = min(len(group_cols), 2)
    for g, c in enumerate(group_cols[:2]):
        d.group_cols[g], d.group_src[g] = colref(c)
    d.naggs = len(aggs)
    kinds = []
    filters = []                 # distinct predicate lists, in order
    for a, spec in enumerate(aggs):
        if isinstance(spec, (tuple, list)) and spec[0] == "filter":
            _tag, spec, fpreds = spec
            key = tuple((colref(c), int(lo), int(hi))
                        for c, lo, hi in fpreds)
            if len(key) > PLAN_MAX_FILTER_PREDS:
                raise ValueError(
                    f"aggregate {a}: a filter holds at most "
                    f"{PLAN_MAX_FILTER_PREDS} predicates")
            if key not in filters:
                if len(filters) == PLAN_MAX_FILTERS:
                    raise ValueError(
                        f"aggregate {a}: more than {PLAN_MAX_FILTERS} "
                        "distinct filters in one plan")
                filters.append(key)
            d.aggs[a].filter = 1 + filters.index(key)
        if spec == "count" or spec == ("count",):
            d.aggs[a].kind = AGG_COUNT_STAR
            d.aggs[a].nfactors = 0
        elif spec[0] == "count_distinct":
            # one plain column; a factor LIST [(col, mod), ...] is passed
            # through so the engine's rejections are reachable
            fs = (list(spec[1]) if isinstance(spec[1], list)
                  else [(spec[1], "id")])
            d.aggs[a].kind = AGG_COUNT_DISTINCT
            d.aggs[a].nfactors = len(fs)
            for f, (c, m) in enumerate(fs):
                d.aggs[a].col[f], d.aggs[a].src[f] = colref(c)
                d.aggs[a].mod[f] = mods[m]
        elif spec[0] == "count":
            d.aggs[a].kind = AGG_COUNT_COL
            d.aggs[a].nfactors = 1
            d.aggs[a].col[0], d.aggs[a].src[0] = colref(spec[1])
            d.aggs[a].mod[0] = 0
        elif spec[0] in ("min", "max"):
            # exactly one factor; a factor LIST is passed through
            # so the engine's nfactors != 1 rejection is reachable
            fs = ([spec[1]] if len(spec[1]) == 2 and
                  isinstance(spec[1][1], str) else list(spec[1]))
            d.aggs[a].kind = AGG_MIN if spec[0] == "min" else AGG_MAX
            d.aggs[a].nfactors = len(fs)
            for f, (c, m) in enumerate(fs):
                d.aggs[a].col[f], d.aggs[a].src[f] = colref(c)
                d.aggs[a].mod[f] = mods[m]
        else:
            assert spec[0] in ("sum", "avg"), spec
            d.aggs[a].kind = AGG_SUM if spec[0] == "sum" else AGG_AVG
            d.aggs[a].nfactors = len(spec[1])
            for f, (c, m) in enumerate(spec[1]):
                d.aggs[a].col[f], d.aggs[a].src[f] = colref(c)
                d.aggs[a].mod[f] = mods[m]
        kinds.append(d.aggs[a].kind)
    d.nfilters = len(filters)
    for k, key in enumerate(filters):
        d.filters[k].npreds = len(key)
        for i, ((name, src), lo, hi) in enumerate(key):
            d.filters[k].preds[i].col = name
            d.filters[k].preds[i].lo = lo
            d.filters[k].preds[i].hi = hi
            d.filters[k].src[i] = src
    if len(order_by) > PLAN_MAX_ORDER:
        raise ValueError(f"order_by holds at most {PLAN_MAX_ORDER} entries")
    d.norder = len(order_by)
    for o, ent in enumerate(order_by):
        what, index, direction = ent[:3]
        desc = {"asc": 0, "desc": 1}[direction]
        # PostgreSQL: NULLS LAST for ASC, NULLS FIRST for DESC
        nulls = ent[3] if len(ent) > 3 else ("nulls_first" if desc
                                             else "nulls_last")
        d.order[o].what = {"key": 0, "agg": 1}[what]
        d.order[o].index = index
        d.order[o].desc = desc
        d.order[o].nulls_first = {"nulls_last": 0, "nulls_first": 1}[nulls]
    d.limit = limit
    d.est_groups = est_groups
    return d, kinds


def build_plan_groups(group_cols=()):
    """The gg_plan_groups (engine_abi.h) of a plan's group columns: columns
    2 and 3, which travel beside the descriptor; ncols = 0 for a plan with at
    most two.  Pure, like build_plan_desc, and takes its column references."""
    if len(group_cols) > PLAN_MAX_GROUP_COLS:
        raise ValueError(
            f"a plan groups by at most {PLAN_MAX_GROUP_COLS} columns")
    g = _PlanGroups()
    rest = list(group_cols[2:])
    g.ncols = len(rest)
    for i, c in enumerate(rest):
        if isinstance(c, str):
            g.cols[i], g.src[i] = c.encode(), 0
        else:
            g.cols[i], g.src[i] = c[1].encode(), 1 + c[0]
    return g


def build_plan_where(joins=(), where=()):
    """The gg_plan_where (engine_abi.h) of a plan's general WHERE clauses:
    `where` holds the clauses of the plan's WHERE (scope 0), and a join
    spec's "where" key those of that join's build filter (scope 1+k, over
    the build table's own columns).  The clauses are ANDed.  Pure: calls
    neither the library nor a GPU.

    A clause is a list of atoms (ORed), or one atom:
      ("range", col, lo, hi)       lo <= col < hi
      ("not_range", col, lo, hi)   col < lo or col >= hi
      ("eq", col, v) | ("ne", col, v)
      ("cmp", a, op, b)            two columns, op in < <= = <> > >=
                                   (> and >= swap the sides)
      ("is_null", col) | ("not_null", col)
      ("in", col, [v, ...])        expands to equalities inside its clause
    and a whole clause ("not_in", col, [v, ...]) expands to one clause per
    value.  `col` is a name or (join_index, name), as in build_plan_desc.
    A comparison over a NULL is not true; is_null is true exactly then.
    More than PLAN_MAX_CLAUSES clauses, PLAN_MAX_ATOMS atoms in a clause or
    PLAN_MAX_WHERE_ATOMS atoms in all raise ValueError."""
    ops = {"<": (ATOM_LT, False), "<=": (ATOM_LE, False),
           "=": (ATOM_EQ, False), "<>": (ATOM_NE, False),
           ">": (ATOM_LT, True), ">=": (ATOM_LE, True)}

    def colref(c):
        if isinstance(c, str):
            return c.encode(), 0
        k, name = c
        return name.encode(), 1 + k

    def atoms_of(a):
        """(kind, (col, src), (col2, src2) | None, lo, hi) per atom"""
        tag = a[0]
        if tag == "range":
            return [(ATOM_RANGE, colref(a[1]), None, int(a[2]), int(a[3]))]
        if tag == "not_range":
            return [(ATOM_NOT_RANGE, colref(a[1]), None, int(a[2]),
                     int(a[3]))]
        if tag == "eq":
            return [(ATOM_RANGE, colref(a[1]), None, int(a[2]),
                     int(a[2]) + 1)]
        if tag == "ne":
            return [(ATOM_NOT_RANGE, colref(a[1]), None, int(a[2]),
                     int(a[2]) + 1)]
        if tag == "in":
            return [(ATOM_RANGE, colref(a[1]), None, int(v), int(v) + 1)
                    for v in a[2]]
        if tag == "cmp":
            kind, swap = ops[a[2]]
            x, y = (a[3], a[1]) if swap else (a[1], a[3])
            return [(kind, colref(x), colref(y), 0, 0)]
        if tag == "is_null":
            return [(ATOM_IS_NULL, colref(a[1]), None, 0, 0)]
        if tag == "not_null":
            return [(ATOM_NOT_NULL, colref(a[1]), None, 0, 0)]
        raise ValueError(f"unknown where atom {a!r}")

    def is_atom(c):
        return isinstance(c, tuple) and len(c) > 0 and isinstance(c[0], str)

    clauses = []                 # (scope, [atoms])
    for scope, cl in ([(0, c) for c in where] +
                      [(1 + j, c) for j, spec in enumerate(joins)
                       for c in spec.get("where", ())]):
        if is_atom(cl) and cl[0] == "not_in":
            for v in cl[2]:
                clauses.append((scope, atoms_of(("ne", cl[1], v))))
        elif is_atom(cl):
            clauses.append((scope, atoms_of(cl)))
        else:
            clauses.append((scope, [t for a in cl for t in atoms_of(a)]))
    if len(clauses) > PLAN_MAX_CLAUSES:
        raise ValueError(
            f"a plan holds at most {PLAN_MAX_CLAUSES} where clauses")
    if sum(len(atoms) for _s, atoms in clauses) > PLAN_MAX_WHERE_ATOMS:
        raise ValueError(
            f"a plan holds at most {PLAN_MAX_WHERE_ATOMS} where atoms")
    w = _PlanWhere()
    w.nclauses = len(clauses)
    for c, (scope, atoms) in enumerate(clauses):
        if len(atoms) > PLAN_MAX_ATOMS:
            raise ValueError(
                f"where clause {c}: a clause holds at most "
                f"{PLAN_MAX_ATOMS} atoms")
        w.clauses[c].scope = scope
        w.clauses[c].natoms = len(atoms)
        for q, (kind, (col, src), b, lo, hi) in enumerate(atoms):
            t = w.clauses[c].atoms[q]
            t.kind, t.col, t.src, t.lo, t.hi = kind, col, src, lo, hi
            if b is not None:
                t.col2, t.src2 = b
    return w


def build_plan_having(aggs=(), having=()):
    """The gg_plan_having (engine_abi.h) of a plan's HAVING: `having` holds
    clauses, which are ANDed, over the values of the plan's aggregates
    `aggs` (build_plan_desc's list).  Pure: calls neither the library nor a
    GPU.

    A clause is a list of atoms (ORed), or one atom; `a` is an aggregate's
    index in `aggs`:
      ("range", a, lo, hi)         lo <= v < hi
      ("not_range", a, lo, hi)     v < lo or v >= hi
      ("cmp", a, op, v)            op in < <= = <> > >=, as a range with
                                   HAVING_NEG_INF / HAVING_POS_INF for the
                                   open side
      ("in", a, [v, ...])          expands to equalities inside its clause
      ("is_null", a) | ("not_null", a)
    Values are signed 128-bit integers in the aggregate's own scaled units.
    HAVING_NEG_INF as lo and HAVING_POS_INF as hi mean "no test" (so an hi of
    HAVING_POS_INF does not exclude that one value).  A MIN or MAX of a group
    without a non-NULL input is NULL: ranges over it are not true.
    More than PLAN_MAX_HAVING_CLAUSES clauses, PLAN_MAX_HAVING_ATOMS atoms in
    a clause or PLAN_MAX_HAVING_TOTAL in all, an unknown atom, an aggregate
    index outside `aggs`, an AVG, a bound outside 128 bits or a v + 1 that
    leaves them raise ValueError."""
    def is_avg(spec):
        if isinstance(spec, (tuple, list)) and spec and spec[0] == "filter":
            spec = spec[1]
        return isinstance(spec, (tuple, list)) and bool(spec) and \
            spec[0] == "avg"

    def agg(a):
        a = int(a)
        if not 0 <= a < len(aggs):
            raise ValueError(f"having names aggregate {a}, the plan has "
                             f"{len(aggs)}")
        if is_avg(aggs[a]):
            raise ValueError(f"having names aggregate {a}, an AVG")
        return a

    def bound(v):
        v = int(v)
        if not HAVING_NEG_INF <= v <= HAVING_POS_INF:
            raise ValueError(f"having bound {v} outside 128 bits")
        return v

    def succ(v):
        v = bound(v)
        if v == HAVING_POS_INF:
            raise ValueError(f"having value {v}: v + 1 leaves 128 bits")
        return v + 1

    def atoms_of(t):
        """(kind, agg, lo, hi) per atom"""
        tag = t[0]
        if tag == "range":
            return [(HAVING_RANGE, agg(t[1]), bound(t[2]), bound(t[3]))]
        if tag == "not_range":
            return [(HAVING_NOT_RANGE, agg(t[1]), bound(t[2]), bound(t[3]))]
        if tag == "in":
            return [(HAVING_RANGE, agg(t[1]), bound(v), succ(v))
                    for v in t[2]]
        if tag == "cmp":
            a, op, v = agg(t[1]), t[2], t[3]
            if op == "<":
                return [(HAVING_RANGE, a, HAVING_NEG_INF, bound(v))]
            if op == "<=":
                return [(HAVING_RANGE, a, HAVING_NEG_INF, succ(v))]
            if op == "=":
                return [(HAVING_RANGE, a, bound(v), succ(v))]
            if op == "<>":
                return [(HAVING_NOT_RANGE, a, bound(v), succ(v))]
            if op == ">":
                return [(HAVING_RANGE, a, succ(v), HAVING_POS_INF)]
            if op == ">=":
                return [(HAVING_RANGE, a, bound(v), HAVING_POS_INF)]
            raise ValueError(f"unknown having comparison {op!r}")
        if tag == "is_null":
            return [(HAVING_IS_NULL, agg(t[1]), 0, 0)]
        if tag == "not_null":
            return [(HAVING_NOT_NULL, agg(t[1]), 0, 0)]
        raise ValueError(f"unknown having atom {t!r}")

    def is_atom(c):
        return isinstance(c, tuple) and len(c) > 0 and isinstance(c[0], str)

    clauses = [atoms_of(cl) if is_atom(cl)
               else [t for a in cl for t in atoms_of(a)] for cl in having]
    if len(clauses) > PLAN_MAX_HAVING_CLAUSES:
        raise ValueError(
            f"a plan holds at most {PLAN_MAX_HAVING_CLAUSES} having clauses")
    if sum(len(atoms) for atoms in clauses) > PLAN_MAX_HAVING_TOTAL:
        raise ValueError(
            f"a plan holds at most {PLAN_MAX_HAVING_TOTAL} having atoms")
    h = _PlanHaving()
    h.nclauses = len(clauses)
    m64 = (1 << 64) - 1
    for c, atoms in enumerate(clauses):
        if not 0 < len(atoms) <= PLAN_MAX_HAVING_ATOMS:
            raise ValueError(
                f"having clause {c}: a clause holds 1 to "
                f"{PLAN_MAX_HAVING_ATOMS} atoms")
        h.clauses[c].natoms = len(atoms)
        for q, (kind, a, lo, hi) in enumerate(atoms):
            t = h.clauses[c].atoms[q]
            t.kind, t.agg = kind, a
            t.lo_lo, t.lo_hi = lo & m64, lo >> 64
            t.hi_lo, t.hi_hi = hi & m64, hi >> 64
    return h


PLAN_MAX_GROUP_COLS = 4


class _PlanGroups(ctypes.Structure):
    _fields_ = [("cols", ctypes.c_char_p * (PLAN_MAX_GROUP_COLS - 2)),
                ("src", ctypes.c_int8 * (PLAN_MAX_GROUP_COLS - 2)),
                ("ncols", ctypes.c_int)]


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", I64),
                ("total_ms", ctypes.c_double), ("rows_in", I64),
                ("rows_out", I64), ("hbm_bytes_algorithmic", I64)]


COLTYPE = {"int64": 0, "int32": 1, "dec64": 2, "char1": 3}
PIPE_Q1, PIPE_Q3, PIPE_SUMPRICE, PIPE_Q5 = 1, 2, 3, 4

# n_name strings in nationkey order (reference fixture nation.csv)
NATION_NAMES = [
    "ALGERIA", "ARGENTINA", "BRAZIL", "CANADA", "EGYPT", "ETHIOPIA",
    "FRANCE", "GERMANY", "INDIA", "INDONESIA", "IRAN", "IRAQ", "JAPAN",
    "JORDAN", "KENYA", "MOROCCO", "MOZAMBIQUE", "PERU", "CHINA", "ROMANIA",
    "SAUDI ARABIA", "VIETNAM", "RUSSIA", "UNITED KINGDOM", "UNITED STATES"]

_EPOCH = datetime.date(2000, 1, 1)


def pgdate(y, m, d):
    """PG DateADT encoding (int32 days since 2000-01-01)."""
    return (datetime.date(y, m, d) - _EPOCH).days


def PGDate(iso):
    y, m, d = map(int, iso.split("-"))
    return pgdate(y, m, d)


def build_library():
    subprocess.run(["make", "-s", "-C", os.path.join(_DIR, "csrc")],
                   check=True)


def _load():
    if not os.path.exists(_LIB_PATH):
        raise EngineError(
            f"engine library missing: {_LIB_PATH}. Build it with "
            "`make -C greengage_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(_LIB_PATH)
    lib.gg_engine_last_error.restype = ctypes.c_char_p
    lib.gg_engine_build_info.restype = ctypes.c_char_p
    lib.gg_engine_init.argtypes = [ctypes.POINTER(_Config)]
    lib.gg_engine_register_table.argtypes = [
        ctypes.c_char_p, ctypes.POINTER(_ColumnDesc), ctypes.c_int, I64,
        ctypes.POINTER(I32)]
    lib.gg_engine_register_synth.argtypes = [ctypes.c_char_p, U64, I64,
                                             ctypes.POINTER(I32)]
    lib.gg_engine_table_nrows.argtypes = [I32, ctypes.POINTER(I64)]
    lib.gg_engine_fetch_column.argtypes = [I32, ctypes.c_char_p,
                                           ctypes.c_void_p, ctypes.c_size_t]
    lib.gg_engine_compile_pipeline.argtypes = [
        ctypes.POINTER(_PipelineDesc), ctypes.POINTER(I32)]
    lib.gg_engine_execute.argtypes = [I32, ctypes.c_void_p, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_size_t)]
    lib.gg_engine_stats.argtypes = [I32, ctypes.POINTER(KernelStat),
                                    ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.gg_engine_comm_id.argtypes = [ctypes.c_void_p]
    lib.gg_engine_comm_init.argtypes = [ctypes.c_void_p]
    lib.gg_engine_compile_plan.argtypes = [ctypes.POINTER(_PlanDesc),
                                           ctypes.POINTER(I32)]
    lib.gg_engine_compile_plan_where.restype = ctypes.c_int
    lib.gg_engine_compile_plan_where.argtypes = [
        ctypes.POINTER(_PlanDesc), ctypes.POINTER(_PlanWhere),
        ctypes.POINTER(I32)]
    lib.gg_engine_plan_where_size.argtypes = []
    lib.gg_engine_plan_where_size.restype = ctypes.c_size_t
    lib.gg_engine_compile_plan_having.restype = ctypes.c_int
    lib.gg_engine_compile_plan_having.argtypes = [
        ctypes.POINTER(_PlanDesc), ctypes.POINTER(_PlanWhere),
        ctypes.POINTER(_PlanHaving), ctypes.POINTER(I32)]
    lib.gg_engine_plan_having_size.argtypes = []
    lib.gg_engine_plan_having_size.restype = ctypes.c_size_t
    lib.gg_engine_compile_plan_groups.restype = ctypes.c_int
    lib.gg_engine_compile_plan_groups.argtypes = [
        ctypes.POINTER(_PlanDesc), ctypes.POINTER(_PlanWhere),
        ctypes.POINTER(_PlanHaving), ctypes.POINTER(_PlanGroups),
        ctypes.POINTER(I32)]
    lib.gg_engine_plan_groups_size.argtypes = []
    lib.gg_engine_plan_groups_size.restype = ctypes.c_size_t
    lib.gg_engine_plan_group_bits_n.restype = ctypes.c_int
    lib.gg_engine_plan_group_bits_n.argtypes = [
        ctypes.c_int, ctypes.POINTER(I64), ctypes.POINTER(I64),
        ctypes.POINTER(ctypes.c_int)]
    lib.gg_engine_plan_desc_size.argtypes = []
    lib.gg_engine_plan_desc_size.restype = ctypes.c_size_t
    lib.gg_engine_plan_topk_tile.argtypes = []
    lib.gg_engine_plan_topk_tile.restype = ctypes.c_int
    lib.gg_engine_plan_group_bits.argtypes = [
        ctypes.POINTER(I64), ctypes.POINTER(I64),
        ctypes.POINTER(ctypes.c_int)]
    lib.gg_engine_table_set_nulls.argtypes = [I32, ctypes.c_char_p,
                                              ctypes.c_void_p]
    lib.gg_engine_hash_groupby_i64_n.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        I64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, I64,
        ctypes.POINTER(I64)]
    lib.gg_engine_numeric_str.argtypes = [U64, I64, ctypes.c_int,
                                          ctypes.c_char_p]
    lib.gg_engine_radix_sort_u64.argtypes = [ctypes.c_void_p,
                                             ctypes.c_void_p, I64,
                                             ctypes.c_int, ctypes.c_int]
    lib.gg_engine_hash_groupby_i64.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, I64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, I64, ctypes.POINTER(I64)]
    lib.gg_engine_aocs_decode.argtypes = [
        ctypes.c_void_p, I64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int, ctypes.c_void_p, I64, ctypes.POINTER(I64)]
    lib.gg_engine_aocs_decode_text.restype = ctypes.c_int
    lib.gg_engine_aocs_decode_text.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
        ctypes.POINTER(ctypes.c_int64)]
    lib.gg_engine_aocs_decode_ao_text.restype = ctypes.c_int
    lib.gg_engine_aocs_decode_ao_text.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
        ctypes.POINTER(ctypes.c_int64)]
    lib.gg_engine_hash_join_i64_spill.restype = ctypes.c_int
    lib.gg_engine_hash_join_i64_spill.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
    lib.gg_engine_hash_groupby_i64_spill.restype = ctypes.c_int
    lib.gg_engine_hash_groupby_i64_spill.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]
    class _AOCol(ctypes.Structure):
        _fields_ = [("name", ctypes.c_char_p),
                    ("type", ctypes.c_int),
                    ("stream", ctypes.c_void_p),
                    ("stream_len", ctypes.c_int64),
                    ("checksums", ctypes.c_int),
                    ("ao_version", ctypes.c_int),
                    ("dsb_version", ctypes.c_int),
                    ("comptype", ctypes.c_int),
                    ("text_dict", ctypes.c_int),
                    ("nullable", ctypes.c_int)]
    lib.gg_AOCol = _AOCol
    lib.gg_engine_table_text_dict.restype = ctypes.c_int
    lib.gg_engine_table_text_dict.argtypes = [
        ctypes.c_int32, ctypes.c_char_p, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32,
        ctypes.POINTER(ctypes.c_int32)]
    lib.gg_engine_register_table_ao.restype = ctypes.c_int
    lib.gg_engine_register_table_ao.argtypes = [
        ctypes.c_char_p, ctypes.POINTER(_AOCol), ctypes.c_int,
        ctypes.POINTER(ctypes.c_int32)]
    lib.gg_engine_text_dict_encode.restype = ctypes.c_int
    lib.gg_engine_text_dict_encode.argtypes = [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    lib.gg_engine_motion_chunkify.restype = ctypes.c_int
    lib.gg_engine_motion_chunkify.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.gg_engine_motion_dechunkify.restype = ctypes.c_int
    lib.gg_engine_motion_dechunkify.argtypes = [
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
        ctypes.POINTER(ctypes.c_int)]
    lib.gg_engine_memtuple_binding.restype = ctypes.c_int
    lib.gg_engine_memtuple_binding.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
        ctypes.POINTER(ctypes.c_int32)]
    lib.gg_engine_memtuple_binding_large.restype = ctypes.c_int
    lib.gg_engine_memtuple_binding_large.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
        ctypes.POINTER(ctypes.c_int32)]
    lib.gg_engine_memtuple_encode.restype = ctypes.c_int
    lib.gg_engine_memtuple_encode.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
        ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64)]
    lib.gg_engine_memtuple_decode.restype = ctypes.c_int
    lib.gg_engine_memtuple_decode.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64)]
    lib.gg_engine_aocs_decode_ao.restype = ctypes.c_int
    lib.gg_engine_aocs_decode_ao.argtypes = [
        ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int,
        ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64)]
    lib.gg_engine_avg_str.argtypes = [U64, I64, ctypes.c_int, I64,
                                      ctypes.c_char_p]
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _check(rc, what):
    if rc != 0:
        raise EngineError(
            f"{what}: status {rc}: {lib().gg_engine_last_error().decode()}")


def _i128(lo, hi):
    return (hi << 64) | lo


def plan_group_bits(mn, mx):
    """Bit widths of the packed code of a two-column group key whose
    columns range over [mn[g], mx[g]] (mn[g] > mx[g]: no rows), as
    gg_engine_plan_group_bits computes them: (status, (b0, b1)).
    status 0 = the pair fits the 62-bit budget, 5 (GG_ENOTSUP) = it does
    not.  Host arithmetic only: needs no Engine and no GPU."""
    bits = (ctypes.c_int * 2)()
    rc = lib().gg_engine_plan_group_bits((I64 * 2)(*mn), (I64 * 2)(*mx),
                                         bits)
    return rc, (bits[0], bits[1])


def plan_group_bits_n(mn, mx):
    """plan_group_bits for len(mn) = 1..4 group columns
    (gg_engine_plan_group_bits_n): (status, (b0, ...)).  status 0 = the
    columns fit the 62-bit budget, 5 (GG_ENOTSUP) = they do not, 1
    (GG_EINVAL) = a column count outside 1..4.  Host arithmetic only."""
    n = len(mn)
    bits = (ctypes.c_int * max(n, 1))()
    rc = lib().gg_engine_plan_group_bits_n(
        n, (I64 * max(n, 1))(*mn), (I64 * max(n, 1))(*mx), bits)
    return rc, tuple(bits[g] for g in range(n))


def plan_topk_tile():
    """Rows per tile of the device top-k's tournament
    (gg_engine_plan_topk_tile): a constant of the library, no GPU needed."""
    return lib().gg_engine_plan_topk_tile()


class Engine:
    """One engine instance per process (= per GPU = per segment)."""

    def __init__(self, device=0, n_segments=1, segment_id=0):
        cfg = _Config(device=device, n_segments=n_segments,
                      segment_id=segment_id, hbm_limit_bytes=0)
        _check(lib().gg_engine_init(ctypes.byref(cfg)), "engine_init")
        self.n_segments = n_segments
        self.segment_id = segment_id
        self._plan_kinds = {}   # plan handle -> descriptor agg kinds
        self._plan_limit = {}   # plan handle -> limit, where it has one
        self._plan_ngroup = {}  # plan handle -> group columns, where > 2

    def shutdown(self):
        _check(lib().gg_engine_shutdown(), "engine_shutdown")

    # ---- comm (Motion-equivalent RCCL bootstrap) ----
    def comm_id(self):
        buf = ctypes.create_string_buffer(128)
        _check(lib().gg_engine_comm_id(buf), "comm_id")
        return buf.raw

    def comm_init(self, id_bytes):
        buf = ctypes.create_string_buffer(bytes(id_bytes), 128)
        _check(lib().gg_engine_comm_init(buf), "comm_init")

    # ---- tables ----
    def register_synth(self, name, seed=42, sf=1):
        h = I32()
        _check(lib().gg_engine_register_synth(name.encode(), seed, sf,
                                              ctypes.byref(h)),
               f"register_synth({name})")
        return h.value

    def register_table(self, name, cols, nrows):
        """cols: list of (name, typename, numpy_array)."""
        descs = (_ColumnDesc * len(cols))()
        keep = []
        for i, (cname, ctype, arr) in enumerate(cols):
            arr = _ascontig(arr, ctype)
            keep.append(arr)
            descs[i].name = cname.encode()
            descs[i].type = COLTYPE[ctype]
            descs[i].host_data = arr.ctypes.data_as(ctypes.c_void_p)
            descs[i].device_data = None
        h = I32()
        _check(lib().gg_engine_register_table(name.encode(), descs,
                                              len(cols), nrows,
                                              ctypes.byref(h)),
               f"register_table({name})")
        return h.value

    def register_table_ao(self, name, cols):
        """Mount a real AO table: cols = list of (name, typename,
        ao_bytes, checksums, ao_version, dsb_version, comptype)."""
        import numpy as np
        L = lib()
        descs = (L.gg_AOCol * len(cols))()
        keep = []
        for i, col in enumerate(cols):
            cname, ctype, ao, cks, aov, dsbv, ct = col[:7]
            ao = np.ascontiguousarray(ao, np.uint8)
            keep.append(ao)
            descs[i].name = cname.encode()
            descs[i].type = COLTYPE[ctype]
            descs[i].stream = ao.ctypes.data_as(ctypes.c_void_p)
            descs[i].stream_len = len(ao)
            descs[i].checksums = cks
            descs[i].ao_version = aov
            descs[i].dsb_version = dsbv
            descs[i].comptype = ct
            descs[i].text_dict = col[7] if len(col) > 7 else 0
            descs[i].nullable = col[8] if len(col) > 8 else 0
        h = I32()
        _check(L.gg_engine_register_table_ao(name.encode(), descs,
                                             len(cols),
                                             ctypes.byref(h)),
               f"register_table_ao({name})")
        return h.value

    def table_text_dict(self, h, col):
        """Sorted dictionary of a text_dict-mounted column."""
        import numpy as np
        out = np.zeros(1 << 16, np.uint8)
        offs = np.zeros(257, np.int64)
        n = ctypes.c_int32()
        _check(lib().gg_engine_table_text_dict(
            h, col.encode(), out.ctypes.data_as(ctypes.c_void_p),
            len(out), offs.ctypes.data_as(ctypes.c_void_p), 256,
            ctypes.byref(n)), "table_text_dict")
        return [bytes(out[offs[i]:offs[i + 1]]) for i in range(n.value)]

    def table_nrows(self, h):
        n = I64()
        _check(lib().gg_engine_table_nrows(h, ctypes.byref(n)), "nrows")
        return n.value

    def fetch_column(self, h, col_name, dtype):
        import numpy as np
        n = self.table_nrows(h)
        arr = np.empty(n, dtype=dtype)
        _check(lib().gg_engine_fetch_column(
            h, col_name.encode(), arr.ctypes.data_as(ctypes.c_void_p),
            arr.nbytes), f"fetch_column({col_name})")
        return arr

    # ---- pipelines ----
    def compile(self, kind, lineitem=-1, orders=-1, customer=-1,
                supplier=-1, nation=-1, cutoff_date=0, cutoff_hi=0,
                mktsegment=0, regionkey=0, limit_k=10):
        d = _PipelineDesc(kind=kind, lineitem=lineitem, orders=orders,
                          customer=customer, supplier=supplier,
                          nation=nation, cutoff_date=cutoff_date,
                          cutoff_hi=cutoff_hi, mktsegment=mktsegment,
                          regionkey=regionkey, limit_k=limit_k)
        h = I32()
        _check(lib().gg_engine_compile_pipeline(ctypes.byref(d),
                                                ctypes.byref(h)), "compile")
        return h.value

    # ---- generalized pipeline descriptor (v2) ----
    def compile_plan(self, scan_table, preds=(), joins=(), group_cols=(),
                     aggs=(), order_by=(), limit=0, est_groups=0, where=(),
                     having=()):
        """Compile a compositional plan (engine_abi.h gg_plan_desc); the
        arguments are build_plan_desc's, `where` (with the join specs'
        "where" keys) build_plan_where's and `having` build_plan_having's.
        A plan without a clause goes through gg_engine_compile_plan as
        ever, one without a HAVING clause takes the calls it always took,
        and only one with three or four group columns (build_plan_groups)
        goes through gg_engine_compile_plan_groups; its rows are read with
        execute_plan_keys."""
        d, kinds = build_plan_desc(scan_table, preds, joins, group_cols,
                                   aggs, order_by, limit, est_groups)
        w = build_plan_where(joins, where)
        hv = build_plan_having(aggs, having)
        gs = build_plan_groups(group_cols)
        h = I32()
        if gs.ncols:
            _check(lib().gg_engine_compile_plan_groups(
                ctypes.byref(d), ctypes.byref(w) if w.nclauses else None,
                ctypes.byref(hv) if hv.nclauses else None, ctypes.byref(gs),
                ctypes.byref(h)), "compile_plan")
            self._plan_ngroup[h.value] = d.ngroup + gs.ncols
        elif hv.nclauses:
            _check(lib().gg_engine_compile_plan_having(
                ctypes.byref(d), ctypes.byref(w) if w.nclauses else None,
                ctypes.byref(hv), ctypes.byref(h)), "compile_plan")
        elif w.nclauses:
            _check(lib().gg_engine_compile_plan_where(
                ctypes.byref(d), ctypes.byref(w), ctypes.byref(h)),
                "compile_plan")
        else:
            _check(lib().gg_engine_compile_plan(
                ctypes.byref(d), ctypes.byref(h)), "compile_plan")
        self._plan_kinds[h.value] = kinds
        if d.limit > 0:
            self._plan_limit[h.value] = d.limit
        return h.value

    def execute_plan(self, p, max_groups=1 << 16):
        """One (key0, key1, vals) per group, in arena order: by (key0,
        key1), or as the plan's order_by / limit say.  vals holds one entry
        per descriptor aggregate: COUNT, COUNT(DISTINCT), SUM -> int,
        MIN/MAX -> int or None (SQL NULL), AVG -> (sum, count) for
        avg_str."""
        if self._plan_ngroup.get(p, 0) > 2:
            raise ValueError("a plan with more than two group columns is "
                             "read with execute_plan_keys")
        return [(k[0], k[1], v) for k, v in self._execute_plan_rows(
            p, max_groups, 2)]

    def execute_plan_keys(self, p, max_groups=1 << 16):
        """One (keys, vals) per group of any plan, in arena order: keys is
        the tuple of the plan's group keys (all four, or the two of
        execute_plan; a NULL key is PLAN_NULL_KEY), vals as execute_plan's.
        Without an order the rows are sorted by the key tuple."""
        return self._execute_plan_rows(p, max_groups,
                                       max(2, self._plan_ngroup.get(p, 0)))

    def _execute_plan_rows(self, p, max_groups, nkeys):
        kinds = self._plan_kinds.get(p)
        nslots_guess = 8 if kinds is None else max(
            8, sum(2 if k == AGG_AVG else 1 for k in kinds))
        # a limited plan emits at most `limit` rows
        max_groups = min(max_groups, self._plan_limit.get(p, max_groups))
        raw = self.execute_raw(
            p, 16 + max_groups * (8 * nkeys + 16 * nslots_guess))
        ng = int.from_bytes(raw[0:8], "little", signed=True)
        nslots = int.from_bytes(raw[8:12], "little", signed=True)
        if kinds is None:
            kinds = [AGG_SUM] * nslots
        groups = []
        off = 16

        def slot():
            nonlocal off
            lo = int.from_bytes(raw[off:off + 8], "little")
            hi = int.from_bytes(raw[off + 8:off + 16], "little",
                                signed=True)
            off += 16
            return lo, hi

        for _ in range(ng):
            keys = tuple(int.from_bytes(raw[off + 8 * g:off + 8 * g + 8],
                                        "little", signed=True)
                         for g in range(nkeys))
            off += 8 * nkeys
            vals = []
            for k in kinds:
                lo, hi = slot()
                if k in (AGG_MIN, AGG_MAX):
                    # lo = int64 bit pattern, hi = non-NULL inputs
                    vals.append(None if hi == 0 else
                                lo - (1 << 64) if lo >> 63 else lo)
                elif k == AGG_AVG:
                    vals.append(((hi << 64) | lo, slot()[0]))
                else:
                    vals.append((hi << 64) | lo)
            groups.append((keys, vals))
        return groups

    def set_nulls(self, table, col, nulls):
        import numpy as np
        nl = np.ascontiguousarray(nulls, np.uint8)
        _check(lib().gg_engine_table_set_nulls(
            table, col.encode(), nl.ctypes.data_as(ctypes.c_void_p)),
            "set_nulls")

    @staticmethod
    def hash_groupby_n(keys, key_nulls, vals, val_nulls):
        import numpy as np
        keys = np.ascontiguousarray(keys, np.int64)
        vals = np.ascontiguousarray(vals, np.int64)
        kn = (None if key_nulls is None
              else np.ascontiguousarray(key_nulls, np.uint8))
        vn = (None if val_nulls is None
              else np.ascontiguousarray(val_nulls, np.uint8))
        cap = len(keys) if len(keys) else 1
        ok = np.empty(cap, np.int64)
        os_ = np.empty(cap, np.int64)
        oc = np.empty(cap, np.int64)
        ng = I64()
        _check(lib().gg_engine_hash_groupby_i64_n(
            keys.ctypes.data_as(ctypes.c_void_p),
            None if kn is None else kn.ctypes.data_as(ctypes.c_void_p),
            vals.ctypes.data_as(ctypes.c_void_p),
            None if vn is None else vn.ctypes.data_as(ctypes.c_void_p),
            len(keys), ok.ctypes.data_as(ctypes.c_void_p),
            os_.ctypes.data_as(ctypes.c_void_p),
            oc.ctypes.data_as(ctypes.c_void_p), cap,
            ctypes.byref(ng)), "hash_groupby_n")
        n = ng.value
        return ok[:n], os_[:n], oc[:n]

    def execute_raw(self, p, arena_bytes):
        arena = ctypes.create_string_buffer(arena_bytes)
        written = ctypes.c_size_t()
        _check(lib().gg_engine_execute(p, arena, arena_bytes,
                                       ctypes.byref(written)), "execute")
        return arena.raw[:written.value]

    def stats(self, p):
        out = (KernelStat * 32)()
        n = ctypes.c_int()
        _check(lib().gg_engine_stats(p, out, 32, ctypes.byref(n)), "stats")
        return [{
            "name": out[i].name.decode(),
            "launches": out[i].launches,
            "total_ms": out[i].total_ms,
            "rows_in": out[i].rows_in,
            "rows_out": out[i].rows_out,
            "hbm_bytes_algorithmic": out[i].hbm_bytes_algorithmic,
        } for i in range(n.value)]

    # ---- typed result decoding (gg_result.h layouts) ----
    def execute_q1(self, p):
        raw = self.execute_raw(p, 8 + 6 * 72)
        n_groups = int.from_bytes(raw[0:4], "little", signed=True)
        groups = []
        off = 8
        for _ in range(6):
            f = _unpack_q1_group(raw[off:off + 72])
            off += 72
            if f["count"]:
                groups.append(f)
        assert len(groups) == n_groups
        return groups

    def execute_q3(self, p, k=10):
        raw = self.execute_raw(p, 48 + 32 * max(k, 1))
        hdr = {
            "n_out": int.from_bytes(raw[0:8], "little", signed=True),
            "n_groups": int.from_bytes(raw[8:16], "little", signed=True),
            "rev_sum4": _i128(int.from_bytes(raw[16:24], "little"),
                              int.from_bytes(raw[24:32], "little",
                                             signed=True)),
            "group_checksum": int.from_bytes(raw[32:40], "little"),
            "n_join_rows": int.from_bytes(raw[40:48], "little", signed=True),
        }
        rows = []
        off = 48
        for _ in range(hdr["n_out"]):
            b = raw[off:off + 32]
            off += 32
            rows.append({
                "orderkey": int.from_bytes(b[0:8], "little", signed=True),
                "revenue4": _i128(int.from_bytes(b[8:16], "little"),
                                  int.from_bytes(b[16:24], "little",
                                                 signed=True)),
                "orderdate": int.from_bytes(b[24:28], "little", signed=True),
                "shippriority": int.from_bytes(b[28:32], "little",
                                               signed=True),
            })
        return rows, hdr

    def execute_q5(self, p):
        raw = self.execute_raw(p, 8 + 25 * 32)
        n_out = int.from_bytes(raw[0:8], "little", signed=True)
        rows = []
        off = 8
        for _ in range(n_out):
            b = raw[off:off + 32]
            off += 32
            nk = int.from_bytes(b[0:4], "little", signed=True)
            rows.append({
                "nationkey": nk,
                "n_name": NATION_NAMES[nk],
                "count": int.from_bytes(b[8:16], "little", signed=True),
                "revenue4": _i128(int.from_bytes(b[16:24], "little"),
                                  int.from_bytes(b[24:32], "little",
                                                 signed=True)),
            })
        return rows

    def execute_sumprice(self, p):
        raw = self.execute_raw(p, 16)
        return (int.from_bytes(raw[0:8], "little", signed=True),
                int.from_bytes(raw[8:16], "little", signed=True))

    # ---- AOCS datum-stream decode (on-disk columnar blocks) ----
    @staticmethod
    def aocs_decode(stream, version, datumlen, nmax, out_width=8):
        import numpy as np
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        vals = np.empty(nmax, np.int32 if out_width == 4 else np.int64)
        nulls = np.empty(nmax, np.uint8)
        n = I64()
        _check(lib().gg_engine_aocs_decode(
            stream.ctypes.data_as(ctypes.c_void_p), len(stream), version,
            datumlen, vals.ctypes.data_as(ctypes.c_void_p), out_width,
            nulls.ctypes.data_as(ctypes.c_void_p), nmax,
            ctypes.byref(n)), "aocs_decode")
        return vals[:n.value], nulls[:n.value]

    @staticmethod
    def aocs_decode_ao(stream, checksums, ao_version, dsb_version,
                       datumlen, nmax, out_width=8, comptype=0):
        """Decode REAL AO storage blocks: restated header parse +
        CRC32C verify on the host, datum-stream content on the GPU."""
        import numpy as np
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        vals = np.empty(nmax, np.int32 if out_width == 4 else np.int64)
        nulls = np.empty(nmax, np.uint8)
        n = I64()
        _check(lib().gg_engine_aocs_decode_ao(
            stream.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
            len(stream), checksums, ao_version, dsb_version, comptype,
            datumlen,
            vals.ctypes.data_as(ctypes.c_void_p), out_width,
            nulls.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), nmax,
            ctypes.byref(n)), "aocs_decode_ao")
        return vals[:n.value], nulls[:n.value]

    @staticmethod
    def aocs_decode_text(stream, version, nmax):
        """GPU decode of TEXT datum-stream blocks; returns
        (list of bytes, nulls)."""
        import numpy as np
        stream = np.ascontiguousarray(stream, np.uint8)
        offs = np.empty(nmax, np.uint64)
        lens = np.empty(nmax, np.uint32)
        nulls = np.empty(nmax, np.uint8)
        pool = np.empty(len(stream) + 64, np.uint8)
        n, plen = I64(), I64()
        _check(lib().gg_engine_aocs_decode_text(
            stream.ctypes.data_as(ctypes.c_void_p), len(stream), version,
            offs.ctypes.data_as(ctypes.c_void_p),
            lens.ctypes.data_as(ctypes.c_void_p),
            nulls.ctypes.data_as(ctypes.c_void_p), nmax,
            pool.ctypes.data_as(ctypes.c_void_p), len(pool),
            ctypes.byref(n), ctypes.byref(plen)), "aocs_decode_text")
        vals = [bytes(pool[offs[i]:offs[i] + lens[i]])
                for i in range(n.value)]
        return vals, nulls[:n.value].copy()

    @staticmethod
    def aocs_decode_ao_text(stream, checksums, ao_version, dsb_version,
                            nmax, comptype=0):
        """Full AO read path for TEXT columns: header/CRC/codec layer
        on the host, GPU varlena decode."""
        import numpy as np
        stream = np.ascontiguousarray(stream, np.uint8)
        offs = np.empty(nmax, np.uint64)
        lens = np.empty(nmax, np.uint32)
        nulls = np.empty(nmax, np.uint8)
        pool = np.empty(len(stream) * 8 + (1 << 16), np.uint8)
        n, plen = I64(), I64()
        _check(lib().gg_engine_aocs_decode_ao_text(
            stream.ctypes.data_as(ctypes.c_void_p), len(stream),
            checksums, ao_version, dsb_version, comptype,
            offs.ctypes.data_as(ctypes.c_void_p),
            lens.ctypes.data_as(ctypes.c_void_p),
            nulls.ctypes.data_as(ctypes.c_void_p), nmax,
            pool.ctypes.data_as(ctypes.c_void_p), len(pool),
            ctypes.byref(n), ctypes.byref(plen)), "aocs_decode_ao_text")
        vals = [bytes(pool[offs[i]:offs[i] + lens[i]])
                for i in range(n.value)]
        return vals, nulls[:n.value].copy()

    @staticmethod
    def hash_join_spill(build_keys, build_vals, probe_keys,
                        budget_bytes):
        """Spill-tier hash join (unique build keys); returns
        (probe_idx, matched_vals, npartitions)."""
        import numpy as np
        bk = np.ascontiguousarray(build_keys, np.int64)
        bv = np.ascontiguousarray(build_vals, np.int64)
        pk = np.ascontiguousarray(probe_keys, np.int64)
        cap = len(pk) + 1
        oi = np.zeros(cap, np.int64)
        ov = np.zeros(cap, np.int64)
        nm = I64()
        np_ = ctypes.c_int32()
        _check(lib().gg_engine_hash_join_i64_spill(
            bk.ctypes.data_as(ctypes.c_void_p),
            bv.ctypes.data_as(ctypes.c_void_p), len(bk),
            pk.ctypes.data_as(ctypes.c_void_p), len(pk), budget_bytes,
            oi.ctypes.data_as(ctypes.c_void_p),
            ov.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(nm),
            ctypes.byref(np_)), "join_spill")
        return oi[:nm.value], ov[:nm.value], np_.value

    @staticmethod
    def hash_groupby_spill(keys, vals, budget_bytes):
        """Spill-tier group-by: partitions staged to host when the
        input exceeds budget_bytes of device memory; returns
        (keys, sums, counts, npartitions)."""
        import numpy as np
        keys = np.ascontiguousarray(keys, np.int64)
        vals = np.ascontiguousarray(vals, np.int64)
        n = len(keys)
        ok = np.zeros(n + 1, np.int64)
        os_ = np.zeros(n + 1, np.int64)
        oc = np.zeros(n + 1, np.int64)
        ng = I64()
        np_ = ctypes.c_int32()
        _check(lib().gg_engine_hash_groupby_i64_spill(
            keys.ctypes.data_as(ctypes.c_void_p),
            vals.ctypes.data_as(ctypes.c_void_p), n, budget_bytes,
            ok.ctypes.data_as(ctypes.c_void_p),
            os_.ctypes.data_as(ctypes.c_void_p),
            oc.ctypes.data_as(ctypes.c_void_p), n + 1,
            ctypes.byref(ng), ctypes.byref(np_)), "groupby_spill")
        g = ng.value
        return ok[:g], os_[:g], oc[:g], np_.value

    @staticmethod
    def text_dict_encode(values, nulls=None, max_dict=4096):
        """GPU dictionary-encode a list of bytes values; returns
        (codes int32, dict list of bytes).  NULLs -> -1."""
        import numpy as np
        n = len(values)
        blob = b"".join(values)
        offs = np.zeros(n, np.uint64)
        lens = np.zeros(n, np.uint32)
        pos = 0
        for i, v in enumerate(values):
            offs[i] = pos
            lens[i] = len(v)
            pos += len(v)
        pool = (np.frombuffer(blob, np.uint8).copy() if blob
                else np.zeros(1, np.uint8))
        nl = (None if nulls is None
              else np.ascontiguousarray(nulls, np.uint8))
        codes = np.zeros(n, np.int32)
        dcap = pos + 16
        dbytes = np.zeros(dcap, np.uint8)
        doffs = np.zeros(max_dict + 1, np.int64)
        nd = ctypes.c_int32()
        _check(lib().gg_engine_text_dict_encode(
            pool.ctypes.data_as(ctypes.c_void_p),
            offs.ctypes.data_as(ctypes.c_void_p),
            lens.ctypes.data_as(ctypes.c_void_p),
            None if nl is None else
            nl.ctypes.data_as(ctypes.c_void_p), n, max_dict,
            codes.ctypes.data_as(ctypes.c_void_p),
            dbytes.ctypes.data_as(ctypes.c_void_p), dcap,
            doffs.ctypes.data_as(ctypes.c_void_p),
            ctypes.byref(nd)), "text_dict_encode")
        d = [bytes(dbytes[doffs[i]:doffs[i + 1]])
             for i in range(nd.value)]
        return codes, d

    @staticmethod
    def motion_chunkify(tuples, max_chunk=8192, append_eos=True):
        """Frame a MemTuple stream as interconnect tuple chunks."""
        import numpy as np
        tuples = np.ascontiguousarray(tuples, np.uint8)
        cap = len(tuples) + (len(tuples) // 16 + 16) * 8 + 64
        out = np.zeros(cap, np.uint8)
        n = I64()
        _check(lib().gg_engine_motion_chunkify(
            tuples.ctypes.data_as(ctypes.c_void_p), len(tuples),
            max_chunk, int(append_eos),
            out.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n)),
            "motion_chunkify")
        return out[:n.value].copy()

    @staticmethod
    def motion_dechunkify(chunks):
        import numpy as np
        chunks = np.ascontiguousarray(chunks, np.uint8)
        out = np.zeros(len(chunks) + 64, np.uint8)
        n, eos = I64(), ctypes.c_int()
        _check(lib().gg_engine_motion_dechunkify(
            chunks.ctypes.data_as(ctypes.c_void_p), len(chunks),
            out.ctypes.data_as(ctypes.c_void_p), len(out),
            ctypes.byref(n), ctypes.byref(eos)), "motion_dechunkify")
        return out[:n.value].copy(), bool(eos.value)

    @staticmethod
    def memtuple_binding_large(attlen, attalign):
        """Host-only restated LARGE binding layout (CPU-testable)."""
        natts = len(attlen)
        al = (ctypes.c_int32 * natts)(*attlen)
        out = (ctypes.c_int32 * (3 + 5 * natts))()
        _check(lib().gg_engine_memtuple_binding_large(
            natts, al, "".join(attalign).encode(), out),
            "memtuple_binding_large")
        meta = (out[0], out[1], out[2])
        per = [tuple(out[3 + i * 5: 8 + i * 5]) for i in range(natts)]
        return meta, per

    @staticmethod
    def memtuple_binding(attlen, attalign):
        """Host-only restated binding layout (CPU-testable)."""
        natts = len(attlen)
        al = (ctypes.c_int32 * natts)(*attlen)
        out = (ctypes.c_int32 * (3 + 5 * natts))()
        _check(lib().gg_engine_memtuple_binding(
            natts, al, "".join(attalign).encode(), out),
            "memtuple_binding")
        meta = (out[0], out[1], out[2])
        per = [tuple(out[3 + i * 5: 8 + i * 5]) for i in range(natts)]
        return meta, per

    @staticmethod
    def memtuple_encode(attlen, attalign, cols, nulls):
        """Bulk GPU encode of column arrays into a MemTuple stream.
        cols[i]: numpy array with itemsize attlen[i], or a list of
        python bytes for attlen -1 (text); nulls[i]: uint8 array or
        None."""
        import numpy as np

        class _TC(ctypes.Structure):
            _fields_ = [("bytes", ctypes.c_void_p),
                        ("offs", ctypes.c_void_p)]

        natts = len(attlen)
        al = (ctypes.c_int32 * natts)(*attlen)
        nrows = len(cols[0])
        carr, keep = [], []
        for l, c in zip(attlen, cols):
            if l == -1:
                blob = b"".join(c)
                offs = np.zeros(nrows + 1, np.int64)
                pos = 0
                for i, v in enumerate(c):
                    pos += len(v)
                    offs[i + 1] = pos
                bts = (np.frombuffer(blob, np.uint8).copy() if blob
                       else np.zeros(1, np.uint8))
                tc = _TC(bts.ctypes.data_as(ctypes.c_void_p).value,
                         offs.ctypes.data_as(ctypes.c_void_p).value)
                keep += [bts, offs, tc]
                carr.append(tc)
            else:
                carr.append(np.ascontiguousarray(c))
        colp = (ctypes.c_void_p * natts)(
            *[ctypes.addressof(c) if isinstance(c, _TC)
              else c.ctypes.data_as(ctypes.c_void_p).value
              for c in carr])
        narr = [None if n is None else
                np.ascontiguousarray(n, np.uint8) for n in nulls]
        nullp = (ctypes.c_void_p * natts)(
            *[0 if n is None else
              n.ctypes.data_as(ctypes.c_void_p).value for n in narr])
        cap = nrows * (8 + sum(8 + max(x, 2) for x in attlen)) + 64
        for l, c in zip(attlen, cols):
            if l == -1:
                cap += sum(len(v) + 8 for v in c)
        out = np.zeros(cap, np.uint8)
        olen = I64()
        _check(lib().gg_engine_memtuple_encode(
            natts, al, "".join(attalign).encode(), colp, nullp, nrows,
            out.ctypes.data_as(ctypes.c_void_p), cap,
            ctypes.byref(olen)), "memtuple_encode")
        return out[:olen.value].copy()

    @staticmethod
    def memtuple_decode(attlen, attalign, stream, cap_rows):
        """Decode a MemTuple stream; text attrs (attlen -1) come back
        as lists of python bytes."""
        import numpy as np

        class _TO(ctypes.Structure):
            _fields_ = [("offs", ctypes.c_void_p),
                        ("lens", ctypes.c_void_p)]

        natts = len(attlen)
        al = (ctypes.c_int32 * natts)(*attlen)
        stream = np.ascontiguousarray(stream, np.uint8)
        dt = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
        cols, keep = [], []
        for l in attlen:
            if l == -1:
                offs = np.zeros(cap_rows, np.uint64)
                lens = np.zeros(cap_rows, np.uint32)
                to = _TO(offs.ctypes.data_as(ctypes.c_void_p).value,
                         lens.ctypes.data_as(ctypes.c_void_p).value)
                keep.append((offs, lens))
                cols.append(to)
            else:
                cols.append(np.zeros(cap_rows, dt[l]))
        nulls = [np.zeros(cap_rows, np.uint8) for _ in attlen]
        colp = (ctypes.c_void_p * natts)(
            *[ctypes.addressof(c) if isinstance(c, _TO)
              else c.ctypes.data_as(ctypes.c_void_p).value
              for c in cols])
        nullp = (ctypes.c_void_p * natts)(
            *[n.ctypes.data_as(ctypes.c_void_p).value for n in nulls])
        n = I64()
        _check(lib().gg_engine_memtuple_decode(
            natts, al, "".join(attalign).encode(),
            stream.ctypes.data_as(ctypes.c_void_p), len(stream), colp,
            nullp, cap_rows, ctypes.byref(n)), "memtuple_decode")
        out, ki = [], 0
        for l, c in zip(attlen, cols):
            if l == -1:
                offs, lens = keep[ki]
                ki += 1
                out.append([bytes(stream[int(offs[i]):
                                         int(offs[i]) + int(lens[i])])
                            for i in range(n.value)])
            else:
                out.append(c[:n.value])
        return out, [nl[:n.value] for nl in nulls]

    # ---- general hash group-by (arbitrary int64 keys, SUM+COUNT) ----
    @staticmethod
    def hash_groupby(keys, vals):
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        vals = np.ascontiguousarray(vals, dtype=np.int64)
        assert len(keys) == len(vals)
        cap = len(keys) if len(keys) else 1
        ok = np.empty(cap, np.int64)
        os_ = np.empty(cap, np.int64)
        oc = np.empty(cap, np.int64)
        ng = I64()
        _check(lib().gg_engine_hash_groupby_i64(
            keys.ctypes.data_as(ctypes.c_void_p),
            vals.ctypes.data_as(ctypes.c_void_p), len(keys),
            ok.ctypes.data_as(ctypes.c_void_p),
            os_.ctypes.data_as(ctypes.c_void_p),
            oc.ctypes.data_as(ctypes.c_void_p), cap,
            ctypes.byref(ng)), "hash_groupby")
        n = ng.value
        return ok[:n], os_[:n], oc[:n]

    # ---- general sort (ORDER BY operator; LSB radix on GPU) ----
    @staticmethod
    def radix_sort(keys, payload=None, key_bytes=8, descending=False):
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        pp = None
        if payload is not None:
            payload = np.ascontiguousarray(payload, dtype=np.uint64)
            assert len(payload) == len(keys)
            pp = payload.ctypes.data_as(ctypes.c_void_p)
        _check(lib().gg_engine_radix_sort_u64(
            keys.ctypes.data_as(ctypes.c_void_p), pp, len(keys),
            key_bytes, 1 if descending else 0), "radix_sort")
        return keys, payload

    # ---- numeric display (product-side finalize) ----
    @staticmethod
    def numeric_str(val128, scale):
        buf = ctypes.create_string_buffer(80)
        lib().gg_engine_numeric_str(val128 & ((1 << 64) - 1), val128 >> 64,
                                    scale, buf)
        return buf.value.decode()

    @staticmethod
    def avg_str(sum128, sum_scale, count):
        buf = ctypes.create_string_buffer(80)
        lib().gg_engine_avg_str(sum128 & ((1 << 64) - 1), sum128 >> 64,
                                sum_scale, count, buf)
        return buf.value.decode()


def _unpack_q1_group(b):
    return {
        "count": int.from_bytes(b[0:8], "little", signed=True),
        "sum_qty_c": int.from_bytes(b[8:16], "little", signed=True),
        "sum_base_c": int.from_bytes(b[16:24], "little", signed=True),
        "sum_dcol_c": int.from_bytes(b[24:32], "little", signed=True),
        "sum_disc4": _i128(int.from_bytes(b[32:40], "little"),
                           int.from_bytes(b[40:48], "little", signed=True)),
        "sum_charge6": _i128(int.from_bytes(b[48:56], "little"),
                             int.from_bytes(b[56:64], "little", signed=True)),
        "returnflag": chr(b[64]),
        "linestatus": chr(b[65]),
    }


def _ascontig(arr, ctype):
    import numpy as np
    want = {"int64": np.int64, "dec64": np.int64, "int32": np.int32,
            "char1": np.uint8}[ctype]
    return np.ascontiguousarray(arr, dtype=want)
