"""Seeded random descriptors with per-aggregate FILTER predicates, shared
by test_gpu_plan_filter_fuzz.py (which runs them) and
test_plan_filter_cpu.py (which asserts, without an engine, the properties
SEED was chosen for).

16 descriptors from one fixed seed: 0..2 joins of mixed kinds over dense
int64, sparse int64 and int32 build keys, the second join sometimes
chained through a payload column of the first; 0..2 group columns (any
pair of small columns, so packed pairs occur); 1..4 aggregates of all six
kinds, each filtered with probability 1/2 and drawing from 1..3 filters
of 1..3 predicates whose columns come from random valid sources (the
driving table or any INNER join's build table); every column nullable
with probability 1/2.  INNER build keys are unique by construction, so no
descriptor is ever skipped.

Everything here is plain numpy: `tables_of` gives the tables in the
evaluator's form without registering anything.
"""
import numpy as np

from plan_filter_ref import NEG_INF, POS_INF, eval_plan, split

SEED = 20261103
NDESC = 16
MODS = ["id", "sub100", "add100"]
MAX_SLOTS = 8                   # GG_PLAN_MAX_AGGS


def _keys(rng, m, unique):
    """(type name, build keys).  Dense keys take the index-map path,
    sparse and int32 keys hash."""
    style = int(rng.integers(0, 3))
    base = rng.permutation(np.arange(2 * m))[:m]      # unique
    if not unique and m > 3:
        base[m // 2:] = base[:m - m // 2]             # SEMI: duplicates
    if style == 0:
        return "int64", (base + 1).astype(np.int64)
    if style == 1:
        return "int64", ((base - m) * 1000 + 7).astype(np.int64)
    return "int32", ((base - m) * 3 + 1).astype(np.int32)


def _probe(rng, keys, n):
    """probe keys for `keys`: about two thirds of them present"""
    pool = np.concatenate([keys.astype(np.int64), keys.astype(np.int64),
                           keys.astype(np.int64) + 2, [-1, 0, 1 << 40]])
    return rng.choice(pool, n)


def _value_cols(rng, n, prefix):
    cols = []
    for i in range(int(rng.integers(2, 4))):
        if rng.random() < 0.5:
            cols.append((f"{prefix}v{i}", "int32",
                         rng.integers(-5000, 5000, n).astype(np.int32)))
        else:
            cols.append((f"{prefix}v{i}", "int64",
                         rng.integers(-120, 120, n).astype(np.int64)))
    cols.append((f"{prefix}s", "int32",
                 rng.integers(-3, 4, n).astype(np.int32)))
    for i in range(2):
        cols.append((f"{prefix}c{i}", "char1",
                     rng.integers(0, int(rng.integers(2, 5)),
                                  n).astype(np.uint8)))
    return cols


def _nullmap(rng, cols, n):
    return {c: rng.random(n) < rng.uniform(0.02, 0.3)
            for c, _t, _a in cols if rng.random() < 0.5}


def _range(rng, a):
    """a half-open range over the values of array `a`: one-sided, an
    equality [v, v+1), or two-sided"""
    v = a.astype(np.int64)
    lo_v, hi_v = int(v.min()), int(v.max()) + 1
    p = rng.random()
    if p < 0.15:
        return NEG_INF, int(rng.integers(lo_v, hi_v + 1))
    if p < 0.3:
        return int(rng.integers(lo_v, hi_v + 1)), POS_INF
    if p < 0.45:
        e = int(v[int(rng.integers(0, len(v)))])
        return e, e + 1
    a1 = int(rng.integers(lo_v, hi_v + 1))
    b1 = int(rng.integers(lo_v, hi_v + 1))
    return min(a1, b1), max(a1, b1) + 1


def _preds(rng, cols, nmax):
    preds = []
    for _ in range(int(rng.integers(0, nmax + 1))):
        c, _t, a = cols[int(rng.integers(0, len(cols)))]
        preds.append((c,) + _range(rng, a))
    return preds


def gen(rng, it):
    """One random descriptor as plain data: tables[name] = (cols,
    nullmap); joins name their build table by `_tname`."""
    n = int(rng.integers(1, 6_001))
    njoins = int(rng.choice([0, 1, 1, 2, 2]))
    kinds = [("inner" if rng.random() < 0.7 else "semi")
             for _ in range(njoins)]
    tables, joins = {}, []
    dcols = _value_cols(rng, n, "d")
    bcols, bkeys = [], []
    for j in range(njoins):
        m = int(rng.integers(1, 501))
        bkeys.append(_keys(rng, m, unique=kinds[j] == "inner"))
        bcols.append(_value_cols(rng, m, f"b{j}"))
    for j in range(njoins):
        ktype, keys = bkeys[j]
        chained = j == 1 and kinds[0] == "inner" and rng.random() < 0.5
        if chained:
            # the probe key is a payload column of join 0's build table
            bcols[0].append(("nk", "int64",
                             _probe(rng, keys, len(bkeys[0][1]))))
        else:
            dcols.append((f"k{j}", "int64", _probe(rng, keys, n)))
        joins.append({"_tname": f"b{j}", "build_key": "bk",
                      "probe_key": "nk" if chained else f"k{j}",
                      "kind": kinds[j], "probe_src": 1 if chained else 0})
    for j in range(njoins):
        ktype, keys = bkeys[j]
        cols = [("bk", ktype, keys)] + bcols[j]
        tables[f"b{j}"] = (cols, _nullmap(rng, cols, len(keys)))
        joins[j]["preds"] = _preds(rng, bcols[j][:4], 1)
    tables["d"] = (dcols, _nullmap(rng, dcols, n))

    # column pools over every valid source
    srcs = [(None, dcols)] + [(j, bcols[j]) for j in range(njoins)
                              if kinds[j] == "inner"]
    arrays = {}

    def ref(j, name, a):
        r = name if j is None else (j, name)
        arrays[r] = a
        return r

    def plain(c):
        return c != "nk" and not c.startswith("k")

    numeric = [ref(j, c, a) for j, cs in srcs for c, t, a in cs
               if t != "char1" and plain(c)]
    anycol = [ref(j, c, a) for j, cs in srcs for c, t, a in cs if plain(c)]
    small = [ref(j, c, a) for j, cs in srcs for c, t, a in cs
             if c.endswith("s") or t == "char1"]

    def pick(pool):
        return pool[int(rng.integers(0, len(pool)))]

    group = [pick(small) for _ in range(int(rng.integers(0, 3)))]

    def factors():
        return [(pick(numeric), MODS[int(rng.integers(0, 3))])
                for _ in range(int(rng.integers(1, 4)))]

    filters = []
    for _ in range(int(rng.integers(1, 4))):
        fl = []
        for _q in range(int(rng.integers(1, 4))):
            c = pick(anycol)
            fl.append((c,) + _range(rng, arrays[c]))
        filters.append(fl)

    aggs = []
    for _ in range(int(rng.integers(1, 5))):
        kind = int(rng.integers(0, 6))
        if kind == 0:
            a = "count"
        elif kind == 1:
            a = ("count", pick(numeric))
        elif kind == 2:
            a = ("sum", factors())
        elif kind == 5:
            a = ("avg", factors())
        else:
            a = ("min" if kind == 3 else "max",
                 (pick(anycol), MODS[int(rng.integers(0, 3))]))
        if rng.random() < 0.5:
            a = ("filter", a, filters[int(rng.integers(0, len(filters)))])
        aggs.append(a)
    return {"it": it, "n": n, "tables": tables, "joins": joins,
            "preds": _preds(rng, dcols[:4], 2), "group": group,
            "aggs": aggs}


def all_descs():
    rng = np.random.default_rng(SEED)
    return [gen(rng, it) for it in range(NDESC)]


# ---- properties of a descriptor, from the generator alone ----

def references_filter(desc):
    return any(split(a)[1] is not None for a in desc["aggs"])


def filters_on_payload(desc):
    return any(not isinstance(c, str)
               for a in desc["aggs"] if split(a)[1] is not None
               for c, _lo, _hi in split(a)[1])


def slots(desc):
    """accumulator slots of the lowered form (engine_abi.h "accumulator
    budget"): MIN/MAX/AVG add a helper count, shared only between
    aggregates over the same factor columns and sources under the same
    filter"""
    n, helpers = 0, set()
    for a in desc["aggs"]:
        a, f = split(a)
        n += 1
        if a != "count" and a[0] in ("min", "max", "avg"):
            cols = ((a[1][0],) if a[0] != "avg"
                    else tuple(c for c, _m in a[1]))
            helpers.add((cols, None if f is None else repr(f)))
    return n + len(helpers)


def tables_of(desc):
    """{name: (data, nulls)} in the evaluator's form, no engine"""
    out = {}
    for name, (cols, nullmap) in desc["tables"].items():
        n = len(cols[0][2])
        data = {c: np.asarray(a).astype(np.int64) for c, _t, a in cols}
        nulls = {c: np.zeros(n, bool) for c, _t, _a in cols}
        for c, nl in nullmap.items():
            nulls[c] = np.asarray(nl).astype(bool)
        out[name] = (data, nulls)
    return out


def ref_joins(desc, reg, handles=None):
    """join specs in the evaluator's form over `reg` = tables_of(desc)"""
    joins = []
    for j in desc["joins"]:
        bd, bn = reg[j["_tname"]]
        joins.append(dict(j, table=(handles or {}).get(j["_tname"], -1),
                          _data=bd, _nulls=bn, _n=len(bd["bk"])))
    return joins


def expected(desc, reg=None, handles=None):
    reg = reg or tables_of(desc)
    data, nulls = reg["d"]
    return eval_plan(desc["n"], data, nulls, desc["preds"],
                     ref_joins(desc, reg, handles), desc["group"],
                     desc["aggs"])


def has_empty_pair(desc):
    """some (group, filtered aggregate) pair receives no row although the
    group exists: the same plan with every filtered aggregate replaced by
    a filtered COUNT(*) reports a 0"""
    cnt = dict(desc, aggs=[("filter", "count", split(a)[1])
                           for a in desc["aggs"] if split(a)[1] is not None])
    if not cnt["aggs"]:
        return False
    return any(v == 0 for _k0, _k1, vals in expected(cnt) for v in vals)
