"""Seeded random-descriptor fuzz over all six aggregate kinds.

The table, predicate and join generators follow test_gpu_plan_fuzz.py
(random column types and nullability, 0..3 scan conjuncts, 0..2 hash
SEMI-joins over dense and sparse key ranges, group by 0/1/2 columns);
the aggregate list draws 1..4 of COUNT(*) / COUNT(col) / SUM / MIN /
MAX / AVG.  Each plan is checked bit-exactly against plan_minmax_ref,
then executed a second time: plans with 8 or fewer observed groups
re-run on the baked-codes kernel and must return the identical result.
Row counts stay small (driving table <= 40,000 rows) so an iteration
costs milliseconds.
"""
import os

import numpy as np
import pytest

from plan_minmax_ref import NEG_INF, POS_INF, eval_plan, register

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


TYPES = ["int64", "int32", "dec64", "char1"]


def _mk_table(eng, rng, name, nrows, want_char1=0):
    """Random table: 1 join-key col, 2-4 value cols, optional char1
    group cols, each col independently nullable."""
    cols = []
    # join key: dense-ish (dense bitmap path) or sparse/negative (hash)
    style = rng.integers(0, 3)
    if style == 0:
        k = rng.integers(0, max(1, nrows // 2), nrows)
    elif style == 1:
        k = rng.integers(0, nrows * 64, nrows)       # > 8x rows: hash
    else:
        k = rng.integers(-1000, 1000, nrows)          # negative: hash
    cols.append(("k", "int64", k.astype(np.int64)))

    for i in range(int(rng.integers(2, 5))):
        tname = TYPES[int(rng.integers(0, len(TYPES)))]
        if tname == "char1":
            a = rng.integers(0, 256, nrows).astype(np.uint8)
        elif tname == "int32":
            a = rng.integers(-5000, 5000, nrows).astype(np.int32)
        else:
            a = rng.integers(-120, 120, nrows).astype(np.int64)
        cols.append((f"v{i}", tname, a))
    for i in range(want_char1):
        # small random alphabet: 2x2 .. 6x6 group grids, so repeats
        # sometimes cross the <=8-group bake threshold
        a = rng.integers(0, int(rng.integers(2, 7)),
                         nrows).astype(np.uint8)
        cols.append((f"g{i}", "char1", a))

    nullmap = {}
    for cname, _t, _a in cols:
        if rng.random() < 0.35:
            nullmap[cname] = rng.random(nrows) < rng.uniform(0.02, 0.3)
    t, data, nulls = register(eng, name, cols, nullmap)
    return t, cols, data, nulls


def _rand_preds(rng, cols, nmax):
    preds = []
    for _ in range(int(rng.integers(0, nmax + 1))):
        cname, _tname, a = cols[int(rng.integers(0, len(cols)))]
        vals = a.astype(np.int64)
        lo_v, hi_v = int(vals.min()), int(vals.max()) + 1
        # random sub-range, sometimes one-sided / empty / full
        p = rng.random()
        if p < 0.1:
            lo, hi = NEG_INF, int(rng.integers(lo_v, hi_v + 1))
        elif p < 0.2:
            lo, hi = int(rng.integers(lo_v, hi_v + 1)), POS_INF
        elif p < 0.25:
            lo, hi = hi_v + 5, hi_v + 6   # selects nothing
        else:
            a1 = int(rng.integers(lo_v, hi_v + 1))
            b1 = int(rng.integers(lo_v, hi_v + 1))
            lo, hi = min(a1, b1), max(a1, b1)
        preds.append((cname, lo, hi))
    return preds


MODS = ["id", "sub100", "add100"]


def _rand_aggs(rng, cols):
    """1..4 aggregates from all six kinds.  SUM/AVG/COUNT(col) draw
    numeric columns like the older fuzz; MIN/MAX draw any column,
    char1 included."""
    numeric = [c[0] for c in cols if c[1] != "char1"]
    anycol = [c[0] for c in cols]

    def factors():
        return [(numeric[int(rng.integers(0, len(numeric)))],
                 MODS[int(rng.integers(0, 3))])
                for _ in range(int(rng.integers(1, 4)))]

    aggs = []
    for _ in range(int(rng.integers(1, 5))):
        kind = int(rng.integers(0, 6))
        if kind == 0:
            aggs.append("count")
        elif kind == 1:
            aggs.append(("count",
                         numeric[int(rng.integers(0, len(numeric)))]))
        elif kind == 2:
            aggs.append(("sum", factors()))
        elif kind == 5:
            aggs.append(("avg", factors()))
        else:
            aggs.append(("min" if kind == 3 else "max",
                         (anycol[int(rng.integers(0, len(anycol)))],
                          MODS[int(rng.integers(0, 3))])))
    return aggs


def _run_one(eng, rng, it, force_interp=False):
    n = int(rng.integers(1, 40_001))
    t, cols, data, nulls = _mk_table(eng, rng, f"mf{it}_d", n,
                                     want_char1=2)
    preds = _rand_preds(rng, cols[:-2], 3)
    joins = []
    for j in range(int(rng.integers(0, 3))):
        bn = int(rng.integers(1, 10_001))
        bt, bcols, bdata, bnulls = _mk_table(eng, rng, f"mf{it}_b{j}", bn)
        joins.append({"table": bt, "build_key": "k", "probe_key": "k",
                      "preds": _rand_preds(rng, bcols, 2),
                      "_n": bn, "_data": bdata, "_nulls": bnulls})

    gm = int(rng.integers(0, 3))
    # group-1 key: a value column (bounded cardinality)
    group_cols = [] if gm == 0 else (
        [cols[int(rng.integers(1, len(cols) - 2))][0]]
        if gm == 1 else ["g0", "g1"])
    aggs = _rand_aggs(rng, cols)

    def key(g):
        return (g[0], g[1])

    if force_interp:
        os.environ["GG_PLAN_RTC"] = "0"
    try:
        p = eng.compile_plan(
            t, preds=preds,
            joins=[{k: v for k, v in j.items()
                    if not k.startswith("_")} for j in joins],
            group_cols=group_cols, aggs=aggs)
        got = sorted(eng.execute_plan(p, max_groups=1 << 17), key=key)
    finally:
        os.environ.pop("GG_PLAN_RTC", None)

    exp = eval_plan(n, data, nulls, preds, joins, group_cols, aggs)
    assert len(got) == len(exp), \
        f"it={it}: {len(got)} groups vs {len(exp)}"
    for g, e in zip(got, exp):
        assert key(g) == key(e), f"it={it}: key {g} vs {e}"
        assert g[2] == e[2], f"it={it}: {aggs}: vals {g} vs {e}"

    # second execute: plans with <=8 observed groups re-run on the
    # baked-codes kernel — results must be identical
    got2 = sorted(eng.execute_plan(p, max_groups=1 << 17), key=key)
    assert got2 == got, f"it={it}: repeat/baked execute diverged"


def test_plan_minmax_fuzz_rtc(eng):
    rng = np.random.default_rng(20261020)
    for it in range(24):
        _run_one(eng, rng, it)


def test_plan_minmax_fuzz_interpreted(eng):
    rng = np.random.default_rng(4242)
    for it in range(8):
        _run_one(eng, rng, 100 + it, force_interp=True)
