"""MIN/MAX/AVG plans at world 2 on ONE GPU over the shm transport.

Launched exactly like test_gpu_multiproc.py launches its worker.  Each
rank aggregates its own shard; exec_plan's cross-segment combine must
merge MIN/MAX words by min/max and sums/counts by addition.  This is
the only place that merge runs: a combine that ADDED the encoded words
would pass every single-rank test.  The shards are built so the global
MIN lives on rank 0 and the global MAX on rank 1, one group exists on
rank 1 only, and one group is all-NULL on rank 0.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_minmax_worker import AGGS, NROWS, make_shard
from plan_minmax_ref import canon, eval_plan

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_minmax_worker.py")


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
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        if p.returncode != 0:
            fail.append(f"rank {r} rc={p.returncode}:\n"
                        f"{out.decode(errors='replace')[-2000:]}")
    assert not fail, "\n".join(fail)
    return [json.load(open(o)) for o in outs]


def test_world2_minmax_avg_combine(tmp_path):
    results = run_world(2, tmp_path)

    # reference over the concatenation of the two shards
    shards = [make_shard(r) for r in range(2)]
    data = {c: np.concatenate([np.asarray(s[0][i][2]).astype(np.int64)
                               for s in shards])
            for i, (c, _t, _a) in enumerate(shards[0][0])}
    nulls = {c: np.zeros(2 * NROWS, bool) for c in data}
    nulls["v"] = np.concatenate([s[1]["v"] for s in shards])
    preds = [("w", -100, 110)]
    exp_g = canon(eval_plan(2 * NROWS, data, nulls, preds, [], ["k"],
                            AGGS))
    exp_0 = canon(eval_plan(2 * NROWS, data, nulls, preds, [], [], AGGS))

    # the shards are shaped as the docstring says
    assert [g[0] for g in exp_g] == [0, 1, 2, 3, 4, 5]
    v0 = data["v"][:NROWS][~nulls["v"][:NROWS]]
    v1 = data["v"][NROWS:][~nulls["v"][NROWS:]]
    assert v0.max() < v1.min()

    for r in results:
        # every rank holds the globally-combined result, first execute
        # and baked repeat alike
        assert r["grouped"] == exp_g
        assert r["grouped_repeat"] == exp_g
        assert r["global"] == exp_0
        assert r["global_repeat"] == exp_0
