"""Seeded random descriptors with LEFT OUTER and ANTI joins, shared by
test_gpu_plan_outer_fuzz.py (which runs them) and test_plan_outer_cpu.py
(which asserts, without an engine, the properties SEED was chosen for).

16 descriptors from one fixed seed, built from plan_filter_gen's parts:
1..2 joins of all four kinds (LEFT and ANTI favoured) over dense int64,
sparse int64 and int32 build keys, the second join often chained through
a payload column of a first INNER or LEFT join; 0..2 group columns, 1..4
aggregates of all six kinds, filters and columns from every valid source
(the driving table, any INNER or LEFT join's build table); every column
nullable with probability 1/2.  Build keys of INNER and LEFT joins are
unique by construction, so no descriptor is ever refused or skipped.

Everything here is plain numpy (plan_filter_gen.tables_of).
"""
import numpy as np

from plan_filter_gen import (MAX_SLOTS, MODS, _nullmap, _preds, _probe,  # noqa: F401
                             _range, _value_cols, ref_joins, slots,
                             tables_of)
from plan_filter_ref import split
from plan_outer_ref import eval_plan, null_extended

SEED = 20261023
NDESC = 16
KINDS = ["left", "anti", "inner", "semi"]
KIND_P = [0.4, 0.35, 0.15, 0.1]
MAP_KINDS = ("inner", "left")


def _keys(rng, m, unique):
    """(style, type name, build keys): dense int64 keys take the index
    map / bitmap, sparse int64 and int32 keys hash"""
    style = ["dense", "dense", "sparse", "int32"][int(rng.integers(0, 4))]
    base = rng.permutation(np.arange(2 * m))[:m]      # unique
    if not unique:
        base[m // 2:] = base[:m - m // 2]             # SEMI/ANTI: duplicates
    if style == "dense":
        return style, "int64", (base + 1).astype(np.int64)
    if style == "sparse":
        return style, "int64", ((base - m) * 1000 + 7).astype(np.int64)
    return style, "int32", ((base - m) * 3 + 1).astype(np.int32)


def _left_ok(desc):
    """every LEFT join NULL-extends 10%..90% of the surviving rows"""
    reg = tables_of(desc)
    data, nulls = reg["d"]
    ext = null_extended(desc["n"], data, nulls, desc["preds"],
                        ref_joins(desc, reg))
    return all(live > 0 and 0.1 * live <= e <= 0.9 * live
               for live, e in ext.values())


def gen(rng, it):
    """One random descriptor as plain data (plan_filter_gen.gen's form).
    A draw whose LEFT joins NULL-extend too few or too many rows to test
    both sides is drawn again from the same stream."""
    while True:
        desc = _draw(rng, it)
        if _left_ok(desc):
            return desc


def _draw(rng, it):
    n = int(rng.integers(50, 6_001))
    njoins = int(rng.choice([1, 2, 2, 2]))
    kinds = [KINDS[int(rng.choice(4, p=KIND_P))] for _ in range(njoins)]
    tables, joins = {}, []
    dcols = _value_cols(rng, n, "d")
    bcols, bkeys = [], []
    for j in range(njoins):
        m = int(rng.integers(4, 501))
        bkeys.append(_keys(rng, m, unique=kinds[j] in MAP_KINDS))
        bcols.append(_value_cols(rng, m, f"b{j}"))
    for j in range(njoins):
        style, ktype, keys = bkeys[j]
        chained = j == 1 and kinds[0] in MAP_KINDS and rng.random() < 0.6
        if chained:
            # the probe key is a payload column of join 0's build table
            bcols[0].append(("nk", "int64",
                             _probe(rng, keys, len(bkeys[0][2]))))
        else:
            dcols.append((f"k{j}", "int64", _probe(rng, keys, n)))
        joins.append({"_tname": f"b{j}", "_style": style, "build_key": "bk",
                      "probe_key": "nk" if chained else f"k{j}",
                      "kind": kinds[j], "probe_src": 1 if chained else 0})
    for j in range(njoins):
        _style, ktype, keys = bkeys[j]
        cols = [("bk", ktype, keys)] + bcols[j]
        tables[f"b{j}"] = (cols, _nullmap(rng, cols, len(keys)))
        joins[j]["preds"] = _preds(rng, bcols[j][:4], 1)
    tables["d"] = (dcols, _nullmap(rng, dcols, n))

    # column pools over every valid source
    srcs = [(None, dcols)] + [(j, bcols[j]) for j in range(njoins)
                              if kinds[j] in MAP_KINDS]
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
            "preds": _preds(rng, dcols[:4], 1), "group": group,
            "aggs": aggs}


def all_descs(seed=SEED):
    rng = np.random.default_rng(seed)
    return [gen(rng, it) for it in range(NDESC)]


def expected(desc, reg=None, handles=None):
    reg = reg or tables_of(desc)
    data, nulls = reg["d"]
    return eval_plan(desc["n"], data, nulls, desc["preds"],
                     ref_joins(desc, reg, handles), desc["group"],
                     desc["aggs"])


# ---- properties of the descriptors, from the generator alone ----

def _left_ref(desc, c):
    return (not isinstance(c, str)
            and desc["joins"][c[0]]["kind"] == "left")


def properties(descs):
    """what the 16 descriptors contain, as counts; `extended` lists, per
    LEFT join, (surviving rows, of which NULL-extended)"""
    p = {"left_dense": 0, "left_hash": 0, "anti_bitmap": 0, "anti_hash": 0,
         "chained_left": 0, "chained_left_anti": 0, "group_left": 0,
         "filter_left": 0, "max_slots": 0, "extended": []}
    for d in descs:
        for j, spec in enumerate(d["joins"]):
            dense = spec["_style"] == "dense"
            if spec["kind"] == "left":
                p["left_dense" if dense else "left_hash"] += 1
            if spec["kind"] == "anti":
                p["anti_bitmap" if dense else "anti_hash"] += 1
            src = spec["probe_src"]
            if src and d["joins"][src - 1]["kind"] == "left":
                p["chained_left"] += 1
                p["chained_left_anti"] += spec["kind"] == "anti"
        p["group_left"] += sum(_left_ref(d, c) for c in d["group"])
        seen = []
        for a in d["aggs"]:
            f = split(a)[1]
            if f is not None and f not in seen:
                seen.append(f)
                p["filter_left"] += any(_left_ref(d, c) for c, _l, _h in f)
        p["max_slots"] = max(p["max_slots"], slots(d))
        reg = tables_of(d)
        data, nulls = reg["d"]
        ext = null_extended(d["n"], data, nulls, d["preds"],
                            ref_joins(d, reg))
        p["extended"] += [(d["it"], j) + v for j, v in sorted(ext.items())]
    return p


def properties_hold(p):
    return (p["left_dense"] >= 4 and p["left_hash"] >= 4
            and p["anti_bitmap"] >= 4 and p["anti_hash"] >= 4
            and p["chained_left"] >= 2 and p["chained_left_anti"] >= 1
            and p["group_left"] >= 3 and p["filter_left"] >= 3
            and p["max_slots"] <= MAX_SLOTS
            and all(live > 0 and 0.1 * live <= ext <= 0.9 * live
                    for _it, _j, live, ext in p["extended"]))
