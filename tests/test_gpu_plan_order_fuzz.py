"""Seeded random descriptors under a random ORDER BY / LIMIT / est_groups.

40 seeds; each draws one descriptor from plan_outer_gen's generator (joins
of all four kinds, 0..2 group columns from every source, all six aggregate
kinds, filters, nullable columns), then an order list of 0..4 entries over
its group keys and its aggregates other than AVG, with random directions
and NULL placements (explicit or left to the binding's default), a limit
and a group estimate.  The result must equal plan_order_ref's row for row
and in order, on two executes (the second may run a baked kernel) and once
more under GG_PLAN_TOPK=host.  Even seeds run the generated kernels, odd
seeds the interpreted one.  The failing seed is in the assertion message.
"""
import os

import numpy as np
import pytest

import plan_outer_gen as gen
from plan_filter_ref import split
from plan_order_ref import order_groups
from plan_outer_ref import plan_mode, register, strip

pytestmark = pytest.mark.gpu

SEED0 = 20261101
NSEEDS = 40


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


def draw_order(rng, desc):
    """(order_by, limit, est_groups) for a descriptor"""
    pool = [("key", g) for g in range(len(desc["group"]))]
    pool += [("agg", a) for a, spec in enumerate(desc["aggs"])
             if split(spec)[0][0] != "avg"]
    order_by = []
    for _ in range(int(rng.integers(0, 5))):
        if not pool:
            break
        what, index = pool[int(rng.integers(0, len(pool)))]
        ent = (what, index, ["asc", "desc"][int(rng.integers(0, 2))])
        placement = [None, "nulls_first", "nulls_last"][
            int(rng.integers(0, 3))]
        order_by.append(ent if placement is None else ent + (placement,))
    limit = int(rng.choice([0, 1, 2, 5, 9, 40, 2000]))
    est = int(rng.choice([0, 1, 50, 10 ** 6]))
    return order_by, limit, est


@pytest.mark.parametrize("k", range(NSEEDS))
def test_plan_order_fuzz(eng, k):
    seed = SEED0 + k
    rng = np.random.default_rng(seed)
    desc = gen.gen(rng, k)
    order_by, limit, est = draw_order(rng, desc)
    mode = "rtc" if k % 2 == 0 else "interp"
    reg, handles = {}, {}
    for name, (cols, nullmap) in desc["tables"].items():
        h, data, nulls = register(eng, f"pordf{k}_{name}", cols, nullmap)
        reg[name], handles[name] = (data, nulls), h
    joins = gen.ref_joins(desc, reg, handles)
    exp = order_groups(gen.expected(desc, reg, handles), order_by, limit)
    what = (f"seed {seed}", mode, order_by, limit, est, desc["group"],
            desc["aggs"])
    with plan_mode(mode):
        p = eng.compile_plan(handles["d"], preds=desc["preds"],
                             joins=strip(joins), group_cols=desc["group"],
                             aggs=desc["aggs"], order_by=order_by,
                             limit=limit, est_groups=est)
        runs = []
        for r in range(2):
            runs.append((r, eng.execute_plan(p, max_groups=1 << 12)))
        os.environ["GG_PLAN_TOPK"] = "host"
        try:
            runs.append(("host", eng.execute_plan(p, max_groups=1 << 12)))
        finally:
            del os.environ["GG_PLAN_TOPK"]
    for r, got in runs:
        assert len(got) == len(exp), (what, r, len(got), len(exp))
        for i, (g, e) in enumerate(zip(got, exp)):
            assert g == e, (what, r, i, g, e)
    names = {s["name"] for s in eng.stats(p)}
    ordered = bool(order_by) or limit > 0
    assert ordered == bool(names & {"path_plan_topk_device",
                                    "path_plan_topk_host"}), what
