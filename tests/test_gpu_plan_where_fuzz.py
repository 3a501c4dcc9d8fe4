"""Seeded random-descriptor fuzz over general WHERE clauses.

The 16 descriptors of plan_where_gen (plan_outer_gen draws with scan
clauses, post-join clauses over INNER and LEFT payload columns, comparisons
mixing sources, and build-scope clauses on joins of all four kinds) each run
on the generated kernels and on the interpreted kernel, three executes each
(the baked kernel takes over where one is made), and must match
plan_where_ref.eval_plan bit for bit.  No descriptor is skipped.

What the seed was chosen for is asserted without a GPU in
test_plan_where_cpu.py.
"""
import pytest

import plan_where_gen as gen
from plan_where_ref import plan_mode, register, strip

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
def test_plan_where_fuzz(eng, descs, it, mode):
    desc = descs[it]
    reg, handles = {}, {}
    for name, (cols, nullmap) in desc["tables"].items():
        h, data, nulls = register(eng, f"pwf{it}_{mode}_{name}", cols,
                                  nullmap)
        reg[name], handles[name] = (data, nulls), h
    joins = gen.ref_joins(desc, reg, handles)
    exp = gen.expected(desc, reg, handles)
    with plan_mode(mode):
        p = eng.compile_plan(handles["d"], preds=desc["preds"],
                             joins=strip(joins), group_cols=desc["group"],
                             aggs=desc["aggs"], where=desc["where"])
        for r in range(3):
            got = sorted(eng.execute_plan(p, max_groups=1 << 12),
                         key=lambda g: (g[0], g[1]))
            what = (it, mode, r, [(j["kind"], j["where"])
                                  for j in desc["joins"]],
                    desc["where"], desc["group"], desc["aggs"])
            assert len(got) == len(exp), (what, len(got), len(exp))
            for g, e in zip(got, exp):
                assert (g[0], g[1]) == (e[0], e[1]), (what, g, e)
                assert g[2] == e[2], (what, g, e)
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    assert "path_plan_where" in paths
    assert ("path_plan_interp" if mode == "interp" else "path_plan_rtc") \
        in paths
