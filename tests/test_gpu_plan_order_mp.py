"""ORDER BY / LIMIT at world 2 on ONE GPU over the shm transport, launched
like test_gpu_plan_outer_mp.py launches its worker.

Every group has rows on both segments, so its aggregates exist only after
the cross-segment combine: the plans are ordered and limited on the host,
after it, and every rank reports plan_order_ref's rows over the
concatenated shards, in order, on all three executes.  A top-k taken per
segment before the combine would be wrong, and the shards are built so that
it would show: neither segment's own top-10 by SUM is the global one.  Two
processes only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_order_worker import AGGS, NGROUPS, NROWS, PLANS, make_shard
from plan_minmax_ref import canon
from plan_order_ref import eval_plan, order_groups

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_order_worker.py")


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
    return run_world(2, tmp_path_factory.mktemp("pord_mp"))


def _groups(shards):
    """the unordered groups over the given shards' rows"""
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


def test_no_segment_knows_the_top_groups(shards, full):
    spec = PLANS["top"]
    top = [g[0] for g in order_groups(full, spec["order_by"],
                                      spec["limit"])]
    for s in shards:
        local = [g[0] for g in order_groups(_groups([s]), spec["order_by"],
                                            spec["limit"])]
        assert set(local) != set(top)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_world2_ordered_and_limited(results, full, name):
    spec = PLANS[name]
    exp = order_groups(full, spec["order_by"], spec["limit"])
    assert len(exp) == (spec["limit"] or NGROUPS)
    for r in results:
        for got in r[name]:
            assert got == canon(exp)
        assert "path_plan_topk_host" in r["paths"][name]
        assert "path_plan_topk_device" not in r["paths"][name]
        assert "path_plan_group_grow" not in r["paths"][name]
