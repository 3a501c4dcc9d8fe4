"""Seeded random-descriptor fuzz over per-aggregate FILTER predicates.

The 16 descriptors of plan_filter_gen (0..2 joins, 0..2 group columns,
1..4 aggregates of all six kinds, each filtered with probability 1/2 from
1..3 filters of 1..3 predicates over random valid sources, nullable
columns) each run on the generated kernels and on the interpreted kernel,
two executes each (the second may run the baked kernel), and must match
plan_filter_ref.eval_plan bit for bit.  No descriptor is skipped.

What the seed was chosen for (at least 10 descriptors reference a filter,
4 filter on a payload column, 3 hold a (group, aggregate) pair that
receives no row, all fit the slot budget) is asserted without a GPU in
test_plan_filter_cpu.py.
"""
import pytest

import plan_filter_gen as gen
from plan_filter_ref import plan_mode, register, strip

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


@pytest.fixture(scope="module")
def descs():
    return gen.all_descs()


@pytest.mark.parametrize("it", range(gen.NDESC))
def test_plan_filter_fuzz(eng, descs, it):
    desc = descs[it]
    reg, handles = {}, {}
    for name, (cols, nullmap) in desc["tables"].items():
        h, data, nulls = register(eng, f"pff{it}_{name}", cols, nullmap)
        reg[name], handles[name] = (data, nulls), h
    joins = gen.ref_joins(desc, reg, handles)
    exp = gen.expected(desc, reg, handles)
    for mode in ("rtc", "interp"):
        with plan_mode(mode):
            p = eng.compile_plan(handles["d"], preds=desc["preds"],
                                 joins=strip(joins),
                                 group_cols=desc["group"], aggs=desc["aggs"])
            for r in range(2):
                got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                             key=lambda g: (g[0], g[1]))
                what = (it, mode, r, desc["group"], desc["aggs"])
                assert len(got) == len(exp), (what, len(got), len(exp))
                for g, e in zip(got, exp):
                    assert (g[0], g[1]) == (e[0], e[1]), (what, g, e)
                    assert g[2] == e[2], (what, g, e)
