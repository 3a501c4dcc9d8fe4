"""COUNT(DISTINCT) at world 2 on ONE GPU over the shm transport, launched
like test_gpu_plan_having_mp.py launches its worker.

Within every group some values occur on both segments.  The (group key,
value) pairs are combined across the segments by their inner code, which
counts such a value once, and regrouped on the host: every rank reports
plan_distinct_ref's rows over the concatenated shards, in order, on all three
executes.  Distinct counts per segment, added up, would be wrong, and the
shards are built so that it would show.  Two processes only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_distinct_worker import AGGS, NGROUPS, NROWS, PLANS, make_shard
from plan_distinct_ref import eval_plan, pair_count
from plan_having_ref import filter_groups
from plan_minmax_ref import canon
from plan_order_ref import order_groups

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_distinct_worker.py")


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
    return run_world(2, tmp_path_factory.mktemp("pdist_mp"))


def _eval(shards, group_cols, fn=eval_plan):
    """the reference over the given shards' rows"""
    cols = [(c, t, np.concatenate([s[0][i][2] for s in shards]))
            for i, (c, t, _a) in enumerate(shards[0][0])]
    n = len(cols[0][2])
    data = {c: np.asarray(a).astype(np.int64) for c, _t, a in cols}
    nulls = {c: np.zeros(n, bool) for c in data}
    for c in shards[0][1]:
        nulls[c] = np.concatenate([s[1][c] for s in shards]).astype(bool)
    return fn(n, data, nulls, [], [], group_cols, AGGS)


@pytest.fixture(scope="module")
def shards():
    return [make_shard(r) for r in range(2)]


def test_no_segment_sum_is_the_distinct_count(shards):
    full = _eval(shards, ["k"])
    assert len(full) == NGROUPS + 1 and sum(
        g[2][1] for g in full) == 2 * NROWS
    local = [{g[0]: g[2][0] for g in _eval([s], ["k"])} for s in shards]
    # every group has values on both segments, and some of them on both
    assert all(g[0] in local[0] and g[0] in local[1] for g in full)
    assert all(max(local[0][g[0]], local[1][g[0]]) < g[2][0]
               < local[0][g[0]] + local[1][g[0]] for g in full)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_world2_pairs_combine_before_the_regroup(results, shards, name):
    spec = PLANS[name]
    full = _eval(shards, spec["group_cols"])
    npairs = _eval(shards, spec["group_cols"], pair_count)
    surv = filter_groups(full, spec.get("having", ()))
    exp = order_groups(surv, spec.get("order_by", ()), spec.get("limit", 0))
    if "having" in spec:
        assert spec["limit"] < len(surv) < len(full)
    for r in results:
        assert len(r[name]) == 3
        for got in r[name]:
            assert got == canon(exp)
        assert "path_plan_distinct_host" in r["paths"][name]
        assert "path_plan_distinct_device" not in r["paths"][name]
        assert "path_plan_having_device" not in r["paths"][name]
        assert "path_plan_topk_device" not in r["paths"][name]
        assert r["regroup"][name] == [3, 3 * npairs, 3 * len(full)]
