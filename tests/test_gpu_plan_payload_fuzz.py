"""Seeded random-descriptor fuzz over INNER joins with payload columns,
in the style of test_gpu_plan_minmax_fuzz.py.

16 descriptors from one fixed seed: 0..2 joins (joins weighted 1:2:2)
of mixed kinds over dense
int64, sparse int64 (negative keys included) and int32 build keys, the
second join sometimes chained through a payload column of the first;
group by 0..2 columns and 1..4 aggregates of all six kinds whose
columns come from random but valid sources (the driving table or any
INNER join's build table); every column nullable with probability 1/2;
0..2 predicates on the driving table and on each build table.  INNER
build keys are unique by construction (a random subset of a range,
scaled), so no descriptor is ever skipped; SEMI build sides get
duplicates on purpose.

Each descriptor runs on the generated kernels and on the interpreted
kernel, two executes each (the second may run the baked kernel), and
must match plan_payload_ref.eval_plan bit for bit.

The generator needs no engine, so the property the test asserts of the
seed — all 16 descriptors run, at least 6 hold an INNER join whose
payload is actually referenced — was checked on the CPU when SEED was
chosen: it gives 12 such descriptors, 4 of them with a chained join,
3 with no join at all.
"""
import numpy as np
import pytest

from plan_payload_ref import (NEG_INF, POS_INF, eval_plan, plan_mode,
                              register, strip)

pytestmark = pytest.mark.gpu

SEED = 20261027
NDESC = 16
MODS = ["id", "sub100", "add100"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


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


def _probe(rng, keys, n, kind):
    """probe keys for `keys`: about half of them present.  INT64_MIN
    goes to INNER joins only: the SEMI hash probe is known to mistake it
    for a match of an empty slot, which is not this test's
    subject."""
    pool = np.concatenate([keys.astype(np.int64),
                           keys.astype(np.int64) + 2,
                           [-1, 0, 1 << 40],
                           [-(1 << 63)] if kind == "inner" else [-2]])
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


def _preds(rng, cols, nmax):
    preds = []
    for _ in range(int(rng.integers(0, nmax + 1))):
        c, _t, a = cols[int(rng.integers(0, len(cols)))]
        v = a.astype(np.int64)
        lo_v, hi_v = int(v.min()), int(v.max()) + 1
        p = rng.random()
        if p < 0.15:
            lo, hi = NEG_INF, int(rng.integers(lo_v, hi_v + 1))
        elif p < 0.3:
            lo, hi = int(rng.integers(lo_v, hi_v + 1)), POS_INF
        else:
            a1 = int(rng.integers(lo_v, hi_v + 1))
            b1 = int(rng.integers(lo_v, hi_v + 1))
            lo, hi = min(a1, b1), max(a1, b1) + 1
        preds.append((c, lo, hi))
    return preds


def gen(rng, it):
    """One random descriptor as plain data: tables[name] = (cols,
    nullmap); joins name their build table by `_tname`."""
    n = int(rng.integers(1, 20_001))
    njoins = int(rng.choice([0, 1, 1, 2, 2]))
    kinds = [("inner" if rng.random() < 0.65 else "semi")
             for _ in range(njoins)]
    tables, joins = {}, []
    dcols = _value_cols(rng, n, "d")
    bcols = []                                # per join: value columns
    bkeys = []
    for j in range(njoins):
        m = int(rng.integers(1, 2_001))
        ktype, keys = _keys(rng, m, unique=kinds[j] == "inner")
        bkeys.append((ktype, keys))
        bcols.append(_value_cols(rng, m, f"b{j}"))
    for j in range(njoins):
        ktype, keys = bkeys[j]
        m = len(keys)
        chained = j == 1 and kinds[0] == "inner" and rng.random() < 0.5
        if chained:
            # the probe key is a payload column of join 0's build table
            m0 = len(bkeys[0][1])
            bcols[0].append(("nk", "int64",
                             _probe(rng, keys, m0, kinds[j])))
        else:
            dcols.append((f"k{j}", "int64",
                          _probe(rng, keys, n, kinds[j])))
        joins.append({"_tname": f"b{j}", "build_key": "bk",
                      "probe_key": "nk" if chained else f"k{j}",
                      "kind": kinds[j], "probe_src": 1 if chained else 0})
    for j in range(njoins):
        ktype, keys = bkeys[j]
        cols = [("bk", ktype, keys)] + bcols[j]
        tables[f"b{j}"] = (cols, _nullmap(rng, cols, len(keys)))
        joins[j]["preds"] = _preds(rng, bcols[j], 2)
    tables["d"] = (dcols, _nullmap(rng, dcols, n))

    # column pools over every valid source
    srcs = [(None, dcols)] + [(j, bcols[j]) for j in range(njoins)
                              if kinds[j] == "inner"]

    def ref(j, name):
        return name if j is None else (j, name)

    numeric = [ref(j, c) for j, cs in srcs for c, t, _a in cs
               if t != "char1" and c != "nk" and not c.startswith("k")]
    anycol = [ref(j, c) for j, cs in srcs for c, t, _a in cs
              if c != "nk" and not c.startswith("k")]
    small = [ref(j, c) for j, cs in srcs for c, t, _a in cs
             if c.endswith("s") or t == "char1"]
    char1 = [ref(j, c) for j, cs in srcs for c, t, _a in cs if t == "char1"]

    def pick(pool):
        return pool[int(rng.integers(0, len(pool)))]

    gm = int(rng.integers(0, 3))
    group = ([] if gm == 0 else [pick(small)] if gm == 1
             else [pick(char1), pick(char1)])

    def factors():
        return [(pick(numeric), MODS[int(rng.integers(0, 3))])
                for _ in range(int(rng.integers(1, 4)))]

    aggs = []
    for _ in range(int(rng.integers(1, 5))):
        kind = int(rng.integers(0, 6))
        if kind == 0:
            aggs.append("count")
        elif kind == 1:
            aggs.append(("count", pick(numeric)))
        elif kind == 2:
            aggs.append(("sum", factors()))
        elif kind == 5:
            aggs.append(("avg", factors()))
        else:
            aggs.append(("min" if kind == 3 else "max",
                         (pick(anycol), MODS[int(rng.integers(0, 3))])))
    return {"it": it, "n": n, "tables": tables, "joins": joins,
            "preds": _preds(rng, dcols[:4], 2), "group": group,
            "aggs": aggs}


def uses_payload(desc):
    """the descriptor holds an INNER join and reads one of its columns:
    as a group key, a factor, or a chained probe key"""
    refs = list(desc["group"])
    for a in desc["aggs"]:
        if a == "count":
            continue
        if a[0] == "count":
            refs.append(a[1])
        elif a[0] in ("min", "max"):
            refs.append(a[1][0])
        else:
            refs += [c for c, _m in a[1]]
    return (any(not isinstance(r, str) for r in refs) or
            any(j["probe_src"] for j in desc["joins"]))


def all_descs():
    rng = np.random.default_rng(SEED)
    return [gen(rng, it) for it in range(NDESC)]


def _run_one(eng, desc):
    reg = {name: register(eng, f"ppf{desc['it']}_{name}", cols, nullmap)
           for name, (cols, nullmap) in desc["tables"].items()}
    t, data, nulls = reg["d"]
    joins = []
    for j in desc["joins"]:
        bt, bd, bn = reg[j["_tname"]]
        joins.append(dict(j, table=bt, _data=bd, _nulls=bn,
                          _n=len(bd["bk"])))
    exp = eval_plan(desc["n"], data, nulls, desc["preds"], joins,
                    desc["group"], desc["aggs"])
    for mode in ("rtc", "interp"):
        with plan_mode(mode):
            p = eng.compile_plan(t, preds=desc["preds"], joins=strip(joins),
                                 group_cols=desc["group"], aggs=desc["aggs"])
            for r in range(2):
                got = sorted(eng.execute_plan(p, max_groups=1 << 15),
                             key=lambda g: (g[0], g[1]))
                what = (desc["it"], mode, r, desc["group"], desc["aggs"])
                assert len(got) == len(exp), (what, len(got), len(exp))
                for g, e in zip(got, exp):
                    assert (g[0], g[1]) == (e[0], e[1]), (what, g, e)
                    assert g[2] == e[2], (what, g, e)


def test_plan_payload_fuzz(eng):
    descs = all_descs()
    ran = 0
    for desc in descs:
        _run_one(eng, desc)
        ran += 1
    assert ran == NDESC == 16
    assert sum(uses_payload(d) for d in descs) >= 6
