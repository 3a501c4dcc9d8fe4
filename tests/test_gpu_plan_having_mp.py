"""HAVING at world 2 on ONE GPU over the shm transport, launched like
test_gpu_plan_order_mp.py launches its worker.

Every group has rows on both segments, so its aggregates exist only after
the cross-segment combine: the HAVING runs on the host, after it, and every
rank reports plan_having_ref's rows over the concatenated shards, in order,
on all three executes.  A HAVING per segment before the combine would be
wrong, and the shards are built so that it would show both ways: some
groups' SUM passes only combined, others pass on one shard and fail
combined.  Two processes only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_having_worker import AGGS, NGROUPS, NROWS, PLANS, make_shard
from plan_having_ref import filter_groups
from plan_minmax_ref import canon
from plan_order_ref import eval_plan, order_groups

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_having_worker.py")


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
    return run_world(2, tmp_path_factory.mktemp("phav_mp"))


def _groups(shards):
    """the unfiltered groups over the given shards' rows"""
    cols = [(c, t, np.concatenate([s[0][i][2] for s in shards]))
            for i, (c, t, _a) in enumerate(shards[0][0])]
    n = len(cols[0][2])
    data = {c: np.asarray(a).astype(np.int64) for c, _t, a in cols}
    nulls = {c: np.zeros(n, bool) for c in data}
    for c in shards[0][1]:
        nulls[c] = np.concatenate([s[1][c] for s in shards]).astype(bool)
    return eval_plan(n, data, nulls, [], [], ["k"], AGGS)


@pytest.fixture(scope="module")
def shards():
    return [make_shard(r) for r in range(2)]


@pytest.fixture(scope="module")
def full(shards):
    groups = _groups(shards)
    assert len(groups) == NGROUPS and sum(
        g[2][1] for g in groups) == 2 * NROWS
    return groups


def test_no_segment_can_decide_the_having(shards, full):
    having = PLANS["having"]["having"]
    passing = {g[0] for g in filter_groups(full, having)}
    local = [{g[0] for g in filter_groups(_groups([s]), having)}
             for s in shards]
    # pass only after the combine: on no shard alone
    assert len(passing - (local[0] | local[1])) >= NGROUPS // 5
    # pass on one shard, fail combined
    assert len(local[0] - passing) >= NGROUPS // 5
    assert len(passing & local[0] & local[1]) >= NGROUPS // 5
    # and COUNT(*) >= 4 holds on no shard alone
    count = [PLANS["having_count"]["having"][0]]
    assert len(filter_groups(full, count)) == NGROUPS
    assert not any(filter_groups(_groups([s]), count) for s in shards)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_world2_having_after_the_combine(results, full, name):
    spec = PLANS[name]
    surv = filter_groups(full, spec["having"])
    exp = order_groups(surv, spec.get("order_by", ()), spec.get("limit", 0))
    assert 0 < len(surv) < NGROUPS and len(exp) == (
        spec.get("limit") or len(surv))
    for r in results:
        assert len(r[name]) == 3
        for got in r[name]:
            assert got == canon(exp)
        assert "path_plan_having_host" in r["paths"][name]
        assert "path_plan_having_device" not in r["paths"][name]
        assert "path_plan_topk_device" not in r["paths"][name]
