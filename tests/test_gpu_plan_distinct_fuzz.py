"""Seeded random-descriptor fuzz over COUNT(DISTINCT) aggregates.

The 16 descriptors of plan_distinct_gen (plan_outer_gen's tables and joins of
all four kinds, 0..1 group columns of any source, 1..2 DISTINCT aggregates
over one column beside 0..3 others, filters, plan_where_gen's WHERE clauses,
orders and limits) each run twice on the default path and once under
GG_PLAN_DISTINCT=host and must match plan_distinct_ref row for row, in order,
with plan_regroup's counts those of the reference.  No descriptor is skipped:
the last test fails unless all 16 ran, and a descriptor the engine refuses
fails its own.

That every pair fits the packed code, and what the seed covers, is asserted
without a GPU in test_plan_distinct_cpu.py.
"""
import os

import pytest

import plan_distinct_gen as gen
from plan_distinct_ref import register, strip
from plan_order_ref import order_groups

pytestmark = pytest.mark.gpu

RAN = set()


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
def descs():
    return gen.all_descs()


@pytest.mark.parametrize("it", range(gen.NDESC))
def test_plan_distinct_fuzz(eng, descs, it):
    desc = descs[it]
    reg, handles = {}, {}
    for name, (cols, nullmap) in desc["tables"].items():
        h, data, nulls = register(eng, f"pdf{it}_{name}", cols, nullmap)
        reg[name], handles[name] = (data, nulls), h
    joins = gen.ref_joins(desc, reg, handles)
    full = gen.expected(desc, reg, handles)
    npairs = gen.pairs(desc, reg, handles)
    exp = order_groups(full, desc["order_by"], desc["limit"])
    what = (it, [j["kind"] for j in desc["joins"]], desc["where"],
            desc["group"], desc["aggs"], desc["order_by"], desc["limit"])
    # a descriptor the engine refuses raises here and fails the test
    p = eng.compile_plan(handles["d"], preds=desc["preds"],
                         joins=strip(joins), group_cols=desc["group"],
                         aggs=desc["aggs"], where=desc["where"],
                         order_by=desc["order_by"], limit=desc["limit"])
    for path in ("default", "default", "host"):
        if path == "host":
            os.environ["GG_PLAN_DISTINCT"] = "host"
        try:
            got = eng.execute_plan(p, max_groups=max(len(exp), 1))
        finally:
            os.environ.pop("GG_PLAN_DISTINCT", None)
        assert len(got) == len(exp), (what, path, len(got), len(exp))
        for g, e in zip(got, exp):
            assert g == e, (what, path, g, e)
    st = {s["name"]: s for s in eng.stats(p)}
    dev = st.get("path_plan_distinct_device", {"launches": 0})["launches"]
    host = st.get("path_plan_distinct_host", {"launches": 0})["launches"]
    assert (dev, host) == ((2, 1) if npairs > 8 else (0, 3)), what
    assert (st["plan_regroup"]["rows_in"], st["plan_regroup"]["rows_out"]) \
        == (3 * npairs, 3 * len(full)), what
    RAN.add(it)


def test_all_descriptors_ran(eng):
    assert RAN == set(range(gen.NDESC))
