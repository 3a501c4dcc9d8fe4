"""Seeded random-descriptor fuzz over two-column group keys of any type
and source, in the style of test_gpu_plan_payload_fuzz.py (whose key,
probe, NULL-map and predicate generators it shares).

16 descriptors from one fixed seed, each over 3,000-4,000 driving rows:
ALWAYS two group columns, each char1, int32 or int64 at random, from the
driving table or from any INNER join's build table at random, with 2 to
40 distinct values, 1 to 2^20 apart, sitting anywhere in the type's
range (int64 bases up to +-2^40); 0..2 joins of mixed kinds, the second sometimes chained;
1..4 aggregates of all six kinds over random sources; every column
nullable with probability 1/2; 0..2 predicates per table.

Each descriptor runs on the generated kernels and on the interpreted
kernel, two executes each (the second runs the baked kernel where the
plan has at most 8 groups), and must match plan_payload_ref.eval_plan
bit for bit.

The generator needs no engine, so these properties of SEED were checked
on the CPU when it was chosen, and the test asserts them again:
  - no descriptor is over the 62-bit budget, none is skipped;
  - every expected group count is <= 4096, the arena of
    plan_payload_ref.run();
  - at least 12 descriptors take the packed path (not two char1);
  - at least 5 have a payload column as a group key;
  - at least 3 have 1..8 groups.
The seed gives 14 packed, 9 with a payload group key and 4 with 1..8
groups; one descriptor's predicates leave no group at all, the largest
group count is 775 and the widest code takes 54 bits.
"""
import numpy as np
import pytest

from plan_payload_ref import eval_plan, plan_mode, register, strip
from test_gpu_plan_payload_fuzz import _keys, _nullmap, _preds, _probe

pytestmark = pytest.mark.gpu

SEED = 20261103
NDESC = 16
MODS = ["id", "sub100", "add100"]
CARDS = [2, 3, 12, 40, 40]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


def _cols(rng, n, prefix):
    """value columns v*, and one group column of each type: g32 and g64
    hold `card` values spread over a window that starts anywhere"""
    cols = []
    for i in range(int(rng.integers(2, 4))):
        if rng.random() < 0.5:
            cols.append((f"{prefix}v{i}", "int32",
                         rng.integers(-5000, 5000, n).astype(np.int32)))
        else:
            cols.append((f"{prefix}v{i}", "int64",
                         rng.integers(-120, 120, n).astype(np.int64)))
    for name, ty, span in (("g32", "int32", 1 << 30), ("g64", "int64", 1 << 40)):
        card = CARDS[int(rng.integers(0, len(CARDS)))]
        base = int(rng.integers(-span, span))
        step = int(rng.choice([1, 7, 1000, 1 << 20]))
        vals = base + step * rng.permutation(np.arange(3 * card))[:card]
        cols.append((f"{prefix}{name}", ty,
                     rng.choice(vals, n).astype(
                         np.int32 if ty == "int32" else np.int64)))
    cols.append((f"{prefix}gc", "char1",
                 rng.integers(0, int(rng.integers(2, 6)), n).astype(np.uint8)
                 + np.uint8(rng.integers(0, 250))))
    return cols


def gen(rng, it):
    n = int(rng.integers(3000, 4001))
    njoins = int(rng.choice([0, 1, 1, 2, 2]))
    kinds = [("inner" if rng.random() < 0.7 else "semi")
             for _ in range(njoins)]
    tables, joins = {}, []
    dcols = _cols(rng, n, "d")
    bcols, bkeys = [], []
    for j in range(njoins):
        m = int(rng.integers(1, 1_001))
        bkeys.append(_keys(rng, m, unique=kinds[j] == "inner"))
        bcols.append(_cols(rng, m, f"b{j}"))
    for j in range(njoins):
        ktype, keys = bkeys[j]
        chained = j == 1 and kinds[0] == "inner" and rng.random() < 0.5
        if chained:
            bcols[0].append(("nk", "int64",
                             _probe(rng, keys, len(bkeys[0][1]), kinds[j])))
        else:
            dcols.append((f"k{j}", "int64", _probe(rng, keys, n, kinds[j])))
        joins.append({"_tname": f"b{j}", "build_key": "bk",
                      "probe_key": "nk" if chained else f"k{j}",
                      "kind": kinds[j], "probe_src": 1 if chained else 0})
    for j in range(njoins):
        ktype, keys = bkeys[j]
        cols = [("bk", ktype, keys)] + bcols[j]
        tables[f"b{j}"] = (cols, _nullmap(rng, cols, len(keys)))
        joins[j]["preds"] = _preds(rng, bcols[j][:2], 2)
    tables["d"] = (dcols, _nullmap(rng, dcols, n))

    srcs = [(None, dcols)] + [(j, bcols[j]) for j in range(njoins)
                              if kinds[j] == "inner"]

    def ref(j, name):
        return name if j is None else (j, name)

    def named(part):
        return [ref(j, c) for j, cs in srcs for c, _t, _a in cs if part in c]

    numeric, groupable = named("v"), named("g")

    def pick(pool):
        return pool[int(rng.integers(0, len(pool)))]

    group = [pick(groupable), pick(groupable)]

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
                         (pick(numeric + groupable),
                          MODS[int(rng.integers(0, 3))])))
    return {"it": it, "n": n, "tables": tables, "joins": joins,
            "preds": _preds(rng, dcols[:2], 2), "group": group,
            "aggs": aggs}


def all_descs():
    rng = np.random.default_rng(SEED)
    return [gen(rng, it) for it in range(NDESC)]


def _column(desc, c):
    """(type, array) of group column reference c"""
    tname, name = ("d", c) if isinstance(c, str) else (f"b{c[0]}", c[1])
    return next((t, a) for n, t, a in desc["tables"][tname][0] if n == name)


def bits_of(desc):
    """the packed widths, from the whole columns as the engine ranges them"""
    out = []
    for c in desc["group"]:
        a = _column(desc, c)[1].astype(np.int64)
        out.append((int(a.max()) - int(a.min()) + 1).bit_length())
    return out


def is_packed(desc):
    return any(_column(desc, c)[0] != "char1" for c in desc["group"])


def has_payload_key(desc):
    return any(not isinstance(c, str) for c in desc["group"])


def expected(desc, reg):
    t, data, nulls = reg["d"]
    joins = []
    for j in desc["joins"]:
        bt, bd, bn = reg[j["_tname"]]
        joins.append(dict(j, table=bt, _data=bd, _nulls=bn, _n=len(bd["bk"])))
    return joins, eval_plan(desc["n"], data, nulls, desc["preds"], joins,
                            desc["group"], desc["aggs"])


def _run_one(eng, desc):
    reg = {name: register(eng, f"gkf{desc['it']}_{name}", cols, nullmap)
           for name, (cols, nullmap) in desc["tables"].items()}
    joins, exp = expected(desc, reg)
    assert len(exp) <= 4096, (desc["it"], len(exp))
    for mode in ("rtc", "interp"):
        with plan_mode(mode):
            p = eng.compile_plan(reg["d"][0], preds=desc["preds"],
                                 joins=strip(joins), group_cols=desc["group"],
                                 aggs=desc["aggs"])
            for r in range(2):
                got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                             key=lambda g: (g[0], g[1]))
                what = (desc["it"], mode, r, desc["group"], desc["aggs"])
                assert len(got) == len(exp), (what, len(got), len(exp))
                for g, e in zip(got, exp):
                    assert (g[0], g[1]) == (e[0], e[1]), (what, g, e)
                    assert g[2] == e[2], (what, g, e)
        packed = "path_plan_group_packed" in {s["name"] for s in eng.stats(p)}
        assert packed == is_packed(desc), (desc["it"], mode, desc["group"])
    return len(exp)


def test_plan_groupkeys_fuzz(eng):
    descs = all_descs()
    assert all(sum(bits_of(d)) <= 62 for d in descs)
    ngroups = [_run_one(eng, d) for d in descs]
    assert len(ngroups) == NDESC == 16
    assert sum(is_packed(d) for d in descs) >= 12
    assert sum(has_payload_key(d) for d in descs) >= 5
    assert sum(1 <= g <= 8 for g in ngroups) >= 3
