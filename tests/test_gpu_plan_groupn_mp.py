"""Three packed group columns at world 2 on ONE GPU over the shm transport,
launched like test_gpu_plan_groupkeys_mp.py launches its worker.

The code of a G = 3 plan depends on the value ranges of all three columns, and
each rank sees only its shard.  The ranks agree on the ranges of all columns
before they pack, and accept or refuse TOGETHER: a rank that refused on its
local ranges while the other went on would leave that one waiting in the
combine's collective.  The 120 s timeout turns such a wait into a failure.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_groupn_worker import AGGS, COLS, make_shard, rows
from plan_groupn_ref import NULL_KEY, eval_plan

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_groupn_worker.py")


def run_world(world, tmp_path):
    env = dict(os.environ)
    env["GG_COMM_SHM"] = "1"
    env.setdefault("GG_COMM_SHM_MB", "192")
    idfile = str(tmp_path / f"commid.{world}")
    procs, outs = [], []
    for r in range(world):
        out = str(tmp_path / f"out.{world}.{r}.json")
        outs.append(out)
        procs.append(subprocess.Popen(
            [sys.executable, WORKER, str(r), str(world), idfile, out],
            env=env, cwd=REPO,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    fail = []
    for r, p in enumerate(procs):
        try:
            out, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        if p.returncode != 0:
            fail.append(f"rank {r} rc={p.returncode}:\n"
                        f"{out.decode(errors='replace')[-2000:]}")
    assert not fail, "\n".join(fail)
    return [json.load(open(o)) for o in outs]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    return run_world(2, tmp_path_factory.mktemp("gn_mp"))


def concat(name):
    """the two shards of table `name` as one table in evaluator form"""
    shards = [make_shard(r)[name] for r in range(2)]
    data = {c: np.concatenate([np.asarray(s[0][i][2]).astype(np.int64)
                               for s in shards])
            for i, (c, _t, _a) in enumerate(shards[0][0])}
    nulls = {c: np.concatenate([
        np.asarray(s[1].get(c, np.zeros(len(s[0][0][2]), bool)))
        for s in shards]) for c in data}
    return len(data["v"]), data, nulls, shards


def _ranges(shards):
    """per rank, per group column: (min, max)"""
    return [[(int(s[0][g][2].min()), int(s[0][g][2].max())) for g in range(3)]
            for s in shards]


def test_world2_ranges_of_all_columns_are_agreed(results):
    from greengage_amd import plan_group_bits_n
    n, data, nulls, shards = concat("agree")
    rg = _ranges(shards)
    assert rg[0][2] == (0, 3) and rg[1][2] == (2, 1002)
    local = [plan_group_bits_n([a for a, _b in r], [b for _a, b in r])
             for r in rg]
    assert local[0] == (0, (3, 2, 3)) and local[1] == (0, (3, 2, 10))

    exp = rows(eval_plan(n, data, nulls, [], [], COLS, AGGS))

    # groups on both ranks and groups on one rank only
    def groups(rank):
        lo, hi = rank * (n // 2), (rank + 1) * (n // 2)
        return {tuple(NULL_KEY if nulls[c][i] else int(data[c][i])
                      for c in COLS) for i in range(lo, hi)}
    g0, g1 = groups(0), groups(1)
    assert g0 & g1 and g0 - g1 and g1 - g0
    assert any(k[0] == NULL_KEY for k in g0 & g1)

    for r in results:
        assert r["agree"] == exp
        assert r["agree_repeat"] == exp
        assert r["agree_after"] == exp
        assert {"path_plan_group_packed",
                "path_plan_group_packed_n"} <= set(r["paths"]), r["paths"]


def test_world2_refuses_together(results):
    from greengage_amd import plan_group_bits_n
    _n, _data, _nulls, shards = concat("refuse")
    rg = _ranges(shards)
    # each rank's own ranges fit the budget, their union does not
    for r in rg:
        assert plan_group_bits_n([a for a, _b in r], [b for _a, b in r]) == \
            (0, (31, 30, 1))
    mn = [min(r[g][0] for r in rg) for g in range(3)]
    mx = [max(r[g][1] for r in rg) for g in range(3)]
    assert plan_group_bits_n(mn, mx) == (5, (31, 30, 2))

    for r in results:
        assert len(r["refuse_errors"]) == 2
        for err in r["refuse_errors"]:
            assert err is not None, "the over-budget plan ran"
            assert "status 5:" in err, err
            assert "31 + 30 + 2 bits" in err, err
