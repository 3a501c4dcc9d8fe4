"""Seeded fuzz of HAVING over compiled plans (engine_abi.h gg_plan_having):
40 random plans over one table of about 300 groups, each with random
aggregates (some FILTERed, some AVG, which a HAVING never names), a random
qual within the limits whose constants are drawn from the reference's own
values, and a random order and limit.  test_gpu_plan_having.run_having runs
each on the default path and under GG_PLAN_HAVING=host against
plan_having_ref.  The generator emits only valid plans: no case is skipped.
"""
import random

import numpy as np
import pytest

from plan_having_ref import I128_MAX, I128_MIN, filter_groups
from test_gpu_plan_having import _dup, make_tab, run_having

pytestmark = pytest.mark.gpu

NPLANS = 40
MAX_CLAUSES, MAX_ATOMS, MAX_TOTAL = 4, 4, 8


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


@pytest.fixture(scope="module")
def tab(eng):
    """~300 groups by one nullable int64 key, 1 to ~12 rows each; m is NULL
    on 40% of the rows; SUM(y * z) leaves int64 in the larger groups"""
    rng = np.random.default_rng(6700)
    keys = (rng.permutation(2000)[:300] * 101 - 9000).astype(np.int64)
    k = _dup(rng, keys, 900)
    n = len(k)
    cols = [("k", "int64", k),
            ("x", "int64", rng.integers(-1000, 1000, n).astype(np.int64)),
            ("y", "int64", rng.integers(-3 * 10 ** 9, 3 * 10 ** 9, n).astype(
                np.int64)),
            ("z", "int64", rng.integers(1, 3 * 10 ** 9, n).astype(np.int64)),
            ("m", "int32", rng.integers(-50, 50, n).astype(np.int32))]
    nullmap = {"k": rng.random(n) < 0.01, "m": rng.random(n) < 0.4}
    return make_tab(eng, "phf_tab", cols, nullmap)


BASE = ["count", ("count", "m"), ("sum", [("x", "id")]),
        ("sum", [("y", "id"), ("z", "id")]), ("min", ("m", "id")),
        ("max", ("m", "id")), ("avg", [("x", "id")])]


def _is_avg(a):
    a = a[1] if a[0] == "filter" else a
    return a != "count" and a[0] == "avg"


def gen_plan(seed, full_of):
    """(aggs, having, order_by, limit) of one valid plan"""
    rng = random.Random(seed)
    while True:
        aggs = []
        for _ in range(rng.randint(1, 4)):
            a = rng.choice(BASE)
            if rng.random() < 0.35:
                lo = rng.randrange(-1000, 900)
                a = ("filter", a, [("x", lo, lo + rng.randrange(1, 1200))])
            aggs.append(a)
        usable = [i for i, a in enumerate(aggs) if not _is_avg(a)]
        if usable:
            break
    full = full_of(["k"], aggs)

    def const(a):
        """a constant near the values aggregate a really takes"""
        v = rng.choice(full)[2][a]
        v = 0 if v is None else v
        return v + rng.choice([-1, 0, 0, 1])

    def atoms(budget):
        a = rng.choice(usable)
        tag = rng.choice(["range", "not_range", "cmp", "cmp", "in",
                          "is_null", "not_null"])
        if tag in ("range", "not_range"):
            lo, hi = const(a), const(a)
            if rng.random() < 0.7:
                lo, hi = min(lo, hi), max(lo, hi) + 1
            if rng.random() < 0.15:
                lo = I128_MIN
            if rng.random() < 0.15:
                hi = I128_MAX
            return [(tag, a, lo, hi)], 1
        if tag == "cmp":
            return [("cmp", a, rng.choice(["<", "<=", "=", "<>", ">", ">="]),
                     const(a))], 1
        if tag == "in":
            n = rng.randint(1, min(3, budget))
            return [("in", a, [const(a) for _ in range(n)])], n
        return [(tag, a)], 1

    having, total = [], 0
    for _ in range(rng.randint(1, MAX_CLAUSES)):
        clause, used = [], 0
        want = rng.randint(1, MAX_ATOMS)
        while used < want and total + used < MAX_TOTAL:
            got, n = atoms(min(want - used, MAX_TOTAL - total - used))
            clause += got
            used += n
        if not clause:
            break
        having.append(clause if len(clause) > 1 or rng.random() < 0.5
                      else clause[0])
        total += used
    order_by = []
    for _ in range(rng.choice([0, 0, 1, 2])):
        if rng.random() < 0.3:
            order_by.append(("key", 0, rng.choice(["asc", "desc"]),
                             rng.choice(["nulls_first", "nulls_last"])))
        else:
            order_by.append(("agg", rng.choice(usable),
                             rng.choice(["asc", "desc"]),
                             rng.choice(["nulls_first", "nulls_last"])))
    limit = rng.choice([0, 0, 1, 5, 50, 400])
    return aggs, having, order_by, limit


@pytest.mark.parametrize("seed", range(NPLANS))
def test_fuzz_having(eng, tab, seed):
    from greengage_amd import build_plan_having
    aggs, having, order_by, limit = gen_plan(7000 + seed, tab["full"])
    h = build_plan_having(aggs, having)         # valid, within the limits
    assert 1 <= h.nclauses <= MAX_CLAUSES
    run_having(eng, tab, ["k"], aggs, having, order_by=order_by, limit=limit)


def test_fuzz_covers_the_ground(tab):
    """what the seeds were chosen for, on the reference alone"""
    tags, kinds, sel = set(), set(), []
    ordered = limited = filtered = multi = 0
    for seed in range(NPLANS):
        aggs, having, order_by, limit = gen_plan(7000 + seed, tab["full"])
        full = tab["full"](["k"], aggs)
        sel.append(len(filter_groups(full, having)) / len(full))
        for cl in having:
            for t in ([cl] if isinstance(cl, tuple) else cl):
                tags.add(t[0])
                a = aggs[t[1]]
                a = a[1] if a[0] == "filter" else a
                kinds.add(a if a == "count" else a[0])
        ordered += bool(order_by)
        limited += limit > 0
        filtered += any(a[0] == "filter" for a in aggs)
        multi += len(having) > 1
    assert tags == {"range", "not_range", "cmp", "in", "is_null", "not_null"}
    assert kinds == {"count", "sum", "min", "max"}
    assert ordered >= 10 and limited >= 10 and filtered >= 10 and multi >= 10
    assert sum(0 < s < 1 for s in sel) >= 20, sel
    assert any(s == 0 for s in sel) and any(s > 0.5 for s in sel), sel
