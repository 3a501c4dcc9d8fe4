"""Seeded random-descriptor fuzz over LEFT OUTER and ANTI joins.

The 16 descriptors of plan_outer_gen (1..2 joins of all four kinds over
dense, sparse and int32 keys, chains through a LEFT join's payload, group
columns, factors and filter columns from LEFT sources, nullable columns)
each run on the generated kernels and on the interpreted kernel, three
executes each (the baked kernel takes over where one is made), and must
match plan_outer_ref.eval_plan bit for bit.  No descriptor is skipped.

What the seed was chosen for is asserted without a GPU in
test_plan_outer_cpu.py.
"""
import pytest

import plan_outer_gen as gen
from plan_outer_ref import plan_mode, register, strip

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


@pytest.mark.parametrize("mode", ["rtc", "interp"])
@pytest.mark.parametrize("it", range(gen.NDESC))
def test_plan_outer_fuzz(eng, descs, it, mode):
    desc = descs[it]
    reg, handles = {}, {}
    for name, (cols, nullmap) in desc["tables"].items():
        h, data, nulls = register(eng, f"pof{it}_{mode}_{name}", cols,
                                  nullmap)
        reg[name], handles[name] = (data, nulls), h
    joins = gen.ref_joins(desc, reg, handles)
    exp = gen.expected(desc, reg, handles)
    with plan_mode(mode):
        p = eng.compile_plan(handles["d"], preds=desc["preds"],
                             joins=strip(joins), group_cols=desc["group"],
                             aggs=desc["aggs"])
        for r in range(3):
            got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                         key=lambda g: (g[0], g[1]))
            what = (it, mode, r, [j["kind"] for j in desc["joins"]],
                    desc["group"], desc["aggs"])
            assert len(got) == len(exp), (what, len(got), len(exp))
            for g, e in zip(got, exp):
                assert (g[0], g[1]) == (e[0], e[1]), (what, g, e)
                assert g[2] == e[2], (what, g, e)
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    kinds = {j["kind"] for j in desc["joins"]}
    assert ("path_plan_join_left" in paths) == ("left" in kinds)
    assert ("path_plan_join_anti" in paths) == ("anti" in kinds)
