"""Seeded random-descriptor fuzz over three and four group columns, in the
style of test_gpu_plan_groupkeys_fuzz.py (whose column generator it shares,
with test_gpu_plan_payload_fuzz.py's key, probe, NULL-map and predicate
generators).

16 descriptors from one fixed seed, each over 3,000-4,000 driving rows: three
or four group columns, each char1, int32 or int64 at random, from the driving
table or from any INNER or LEFT join's build table at random; 0..2 joins of
kinds SEMI, INNER and LEFT, the second sometimes chained; 1..4 aggregates of
all six kinds over random sources; every column nullable with probability
1/2; 0..2 predicates per table.

Each descriptor runs on the generated kernels and on the interpreted kernel,
three executes each (the later ones run the baked kernel where the plan has at
most 8 groups), and must match plan_groupn_ref.eval_plan bit for bit.  A
descriptor whose columns take more than 62 bits must be refused with
GG_ENOTSUP at the first execute, naming the widths.

The generator needs no engine, so these properties of SEED were checked on the
CPU when it was chosen (tests/test_plan_groupn_cpu.py asserts them without a
GPU), and the test asserts the first again:
  - at least 12 descriptors are within the 62-bit budget;
  - both G = 3 and G = 4 occur;
  - at least 5 have a payload column as a group key, one of them from a
    LEFT join;
  - every expected group count is <= 4096, the arena of
    plan_groupn_ref.run().
"""
import numpy as np
import pytest

import plan_groupn_ref as ref
from plan_groupn_ref import plan_mode, register, strip
from test_gpu_plan_groupkeys_fuzz import MODS, _cols
from test_gpu_plan_payload_fuzz import _keys, _nullmap, _preds, _probe

pytestmark = pytest.mark.gpu

SEED = 20261021
NDESC = 16
KINDS = ["inner", "inner", "left", "left", "semi"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


def gen(rng, it):
    n = int(rng.integers(3000, 4001))
    njoins = int(rng.choice([0, 1, 1, 2, 2]))
    kinds = [KINDS[int(rng.integers(0, len(KINDS)))] for _ in range(njoins)]
    tables, joins = {}, []
    dcols = _cols(rng, n, "d")
    bcols, bkeys = [], []
    for j in range(njoins):
        m = int(rng.integers(1, 1_001))
        bkeys.append(_keys(rng, m, unique=kinds[j] != "semi"))
        bcols.append(_cols(rng, m, f"b{j}"))
    for j in range(njoins):
        ktype, keys = bkeys[j]
        pk = "semi" if kinds[j] == "semi" else "inner"
        chained = j == 1 and kinds[0] != "semi" and rng.random() < 0.5
        if chained:
            bcols[0].append(("nk", "int64",
                             _probe(rng, keys, len(bkeys[0][1]), pk)))
        else:
            dcols.append((f"k{j}", "int64", _probe(rng, keys, n, pk)))
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
                              if kinds[j] != "semi"]

    def named(part):
        return [(c if j is None else (j, c))
                for j, cs in srcs for c, _t, _a in cs if part in c]

    numeric, groupable = named("v"), named("g")

    def pick(pool):
        return pool[int(rng.integers(0, len(pool)))]

    group = [pick(groupable) for _ in range(int(rng.integers(3, 5)))]

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


def column(desc, c):
    """the whole column group column reference c names"""
    tname, name = ("d", c) if isinstance(c, str) else (f"b{c[0]}", c[1])
    return next(np.asarray(a).astype(np.int64)
                for n, _t, a in desc["tables"][tname][0] if n == name)


def bits_of(desc):
    return ref.widths([column(desc, c) for c in desc["group"]])


def has_payload_key(desc):
    return any(not isinstance(c, str) for c in desc["group"])


def has_left_key(desc):
    return any(not isinstance(c, str) and desc["joins"][c[0]]["kind"] == "left"
               for c in desc["group"])


def _evaluator_tables(desc):
    """every table in the evaluator's form, without an engine"""
    out = {}
    for name, (cols, nullmap) in desc["tables"].items():
        n = len(cols[0][2])
        data = {c: np.asarray(a).astype(np.int64) for c, _t, a in cols}
        nulls = {c: np.zeros(n, bool) for c, _t, _a in cols}
        for c, nl in nullmap.items():
            nulls[c] = np.asarray(nl).astype(bool)
        out[name] = (None, data, nulls)
    return out


def expected(desc, reg=None):
    reg = reg or _evaluator_tables(desc)
    _t, data, nulls = reg["d"]
    joins = []
    for j in desc["joins"]:
        bt, bd, bn = reg[j["_tname"]]
        joins.append(dict(j, table=bt, _data=bd, _nulls=bn, _n=len(bd["bk"])))
    return joins, ref.eval_plan(desc["n"], data, nulls, desc["preds"], joins,
                                desc["group"], desc["aggs"])


def _run_one(eng, desc):
    from greengage_amd import EngineError
    reg = {name: register(eng, f"gnf{desc['it']}_{name}", cols, nullmap)
           for name, (cols, nullmap) in desc["tables"].items()}
    bits = bits_of(desc)
    if sum(bits) > 62:
        for mode in ("rtc", "interp"):
            joins = [dict(j, table=reg[j["_tname"]][0]) for j in desc["joins"]]
            with plan_mode(mode), pytest.raises(EngineError) as ei:
                p = eng.compile_plan(reg["d"][0], preds=desc["preds"],
                                     joins=strip(joins),
                                     group_cols=desc["group"],
                                     aggs=desc["aggs"])
                eng.execute_plan_keys(p, max_groups=16)
            assert "status 5:" in str(ei.value), ei.value
            assert " + ".join(str(b) for b in bits) + " bits" in str(ei.value)
        return None
    joins, exp = expected(desc, reg)
    assert len(exp) <= 4096, (desc["it"], len(exp))
    for mode in ("rtc", "interp"):
        try:
            _p, _e, paths = ref.run(eng, mode, reg["d"][0], reg["d"][1],
                                    reg["d"][2], desc["preds"], joins,
                                    desc["group"], desc["aggs"], exp=exp)
        except AssertionError as e:
            raise AssertionError((desc["it"], mode, desc["group"],
                                  desc["aggs"]) + e.args) from e
        assert "path_plan_group_packed_n" in paths, (desc["it"], mode, paths)
    return len(exp)


def test_plan_groupn_fuzz(eng):
    descs = all_descs()
    ngroups = [_run_one(eng, d) for d in descs]
    assert len(ngroups) == NDESC == 16
    assert sum(g is not None for g in ngroups) >= 12
    assert sum(sum(bits_of(d)) <= 62 for d in descs) == \
        sum(g is not None for g in ngroups)
