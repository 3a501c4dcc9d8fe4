"""Seeded random descriptors with general WHERE clauses, shared by
test_gpu_plan_where_fuzz.py (which runs them) and test_plan_where_cpu.py
(which asserts, without an engine, the properties SEED was chosen for).

16 descriptors from one fixed seed.  Each is a plan_outer_gen draw (1..2
joins of all four kinds over dense, sparse and int32 keys, chains, 0..2 group
columns, 1..4 aggregates of all six kinds, filters, nullable columns) with
clauses added: 1..3 clauses of scope 0 over the driving table and over the
build table of every INNER or LEFT join, comparisons that mix the two
included, and 0..2 clauses in the build scope of each join.  Clauses are
drawn permissive (several ORed atoms) so that rows survive; a draw whose
WHERE keeps no row is drawn again from the same stream, so no descriptor
is ever skipped.

Everything here is plain numpy (plan_filter_gen.tables_of).
"""
import numpy as np

import plan_outer_gen as outer
from plan_filter_gen import _range, ref_joins, tables_of
from plan_where_ref import clauses_of, eval_plan, row_masks

SEED = 20261028
NDESC = 16
MAP_KINDS = ("inner", "left")
CMP_OPS = ["<", "<=", "=", "<>", ">", ">="]


def _atom(rng, pool, arrays, other_pool=None):
    """one random atom over the columns `pool` (arrays[c] = the values); a
    comparison takes its second column from `other_pool`"""
    c = pool[int(rng.integers(0, len(pool)))]
    a = arrays[c].astype(np.int64)
    p = rng.random()
    if p < 0.2:
        return ("range", c) + _range(rng, a)
    if p < 0.35:
        return ("not_range", c) + _range(rng, a)
    if p < 0.45:
        return ("eq", c, int(a[int(rng.integers(0, len(a)))]))
    if p < 0.55:
        return ("ne", c, int(a[int(rng.integers(0, len(a)))]))
    if p < 0.65:
        return ("in", c, [int(v) for v in
                          rng.choice(a, int(rng.integers(2, 4)))])
    if p < 0.85:
        op = other_pool or pool
        other = op[int(rng.integers(0, len(op)))]
        return ("cmp", c, CMP_OPS[int(rng.integers(0, 6))], other)
    return ("is_null" if rng.random() < 0.5 else "not_null", c)


def _clause(rng, pool, arrays, other_pool=None):
    if rng.random() < 0.1:
        c = pool[int(rng.integers(0, len(pool)))]
        a = arrays[c].astype(np.int64)
        return ("not_in", c, [int(v) for v in rng.choice(a, 2)])
    atoms = [_atom(rng, pool, arrays, other_pool)
             for _ in range(int(rng.integers(1, 4)))]
    return atoms[0] if len(atoms) == 1 and rng.random() < 0.5 else atoms


def _add_where(rng, desc):
    dcols = desc["tables"]["d"][0]
    dpool = [c for c, _t, _a in dcols]
    arrays = {c: a for c, _t, a in dcols}
    ppool = []                   # payload columns of the map joins
    for j, spec in enumerate(desc["joins"]):
        bcols = desc["tables"][spec["_tname"]][0]
        barr = {c: a for c, _t, a in bcols}
        spec["where"] = [_clause(rng, list(barr), barr)
                         for _ in range(int(rng.choice([0, 0, 1, 2])))]
        if spec["kind"] in MAP_KINDS:
            for c, _t, a in bcols:
                ppool.append((j, c))
                arrays[(j, c)] = a
    where = []
    for _ in range(int(rng.integers(1, 4))):
        p = rng.random()
        if p < 0.4 or not ppool:
            where.append(_clause(rng, dpool, arrays))
        elif p < 0.65:
            where.append(_clause(rng, ppool, arrays))
        else:
            # comparisons of a driving column with a payload column
            where.append(_clause(rng, dpool, arrays, ppool))
    desc["where"] = where


def masks(desc, reg=None):
    """(rows preds and joins keep, of which the WHERE keeps, ridx)"""
    reg = reg or tables_of(desc)
    data, nulls = reg["d"]
    return row_masks(desc["n"], data, nulls, desc["preds"],
                     ref_joins(desc, reg), desc["where"])


def gen(rng, it):
    """One random descriptor as plain data (plan_filter_gen.gen's form plus
    "where" on the descriptor and on its join specs).  A draw that exceeds
    the extension's limits, or whose WHERE keeps no row, is drawn again from
    the same stream."""
    from greengage_amd import build_plan_where

    while True:
        desc = outer._draw(rng, it)
        _add_where(rng, desc)
        try:
            build_plan_where(desc["joins"], desc["where"])
        except ValueError:
            continue
        if masks(desc)[1].any():
            return desc


def all_descs(seed=SEED):
    rng = np.random.default_rng(seed)
    return [gen(rng, it) for it in range(NDESC)]


def expected(desc, reg=None, handles=None, evaluator=eval_plan):
    reg = reg or tables_of(desc)
    data, nulls = reg["d"]
    return evaluator(desc["n"], data, nulls, desc["preds"],
                     ref_joins(desc, reg, handles), desc["group"],
                     desc["aggs"], desc["where"])


# ---- properties of the descriptors, from the generator alone ----

def _srcs(atom):
    cols = [atom[1]] + ([atom[3]] if atom[0] == "cmp" else [])
    return {0 if isinstance(c, str) else 1 + c[0] for c in cols}


def properties(descs):
    """what the 16 descriptors contain, as counts"""
    from greengage_amd import build_plan_where

    p = {"kinds": set(), "scan": 0, "post": 0, "build": 0, "left_null": 0,
         "mixed": 0, "drops_and_keeps": 0, "empty": 0, "nclauses": 0}
    for d in descs:
        w = build_plan_where(d["joins"], d["where"])
        p["nclauses"] += w.nclauses
        for c in range(w.nclauses):
            for q in range(w.clauses[c].natoms):
                p["kinds"].add(int(w.clauses[c].atoms[q].kind))
        cls = clauses_of(d["where"])
        srcs = [set().union(*[_srcs(a) for a in cl]) for cl in cls]
        p["scan"] += any(s == {0} for s in srcs)
        p["post"] += any(s != {0} for s in srcs)
        p["build"] += any(j.get("where") for j in d["joins"])
        p["mixed"] += any(a[0] == "cmp" and len(_srcs(a)) == 2
                          for cl in cls for a in cl)
        m0, m1, ridx = masks(d)
        left = {1 + j for j, s in enumerate(d["joins"])
                if s["kind"] == "left" and (m0 & (ridx[j] < 0)).any()}
        p["left_null"] += any(s & left for s in srcs)
        p["drops_and_keeps"] += bool((m0 & ~m1).any() and m1.any())
        p["empty"] += not expected(d)
    return p


def properties_hold(p):
    return (p["kinds"] == set(range(8)) and p["scan"] >= 4 and p["post"] >= 4
            and p["build"] >= 4 and p["left_null"] >= 3 and p["mixed"] >= 3
            and p["drops_and_keeps"] >= 12 and p["empty"] == 0)
