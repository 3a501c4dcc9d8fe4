"""Packed two-column group keys at world 2 on ONE GPU over the shm
transport, launched like test_gpu_plan_minmax_mp.py launches its worker.

The packed code depends on the columns' value ranges, and each rank sees
only its shard.  The ranks must therefore agree on the ranges before
they pack — else equal pairs get different codes on different ranks and
the cross-segment combine merges nonsense — and must accept or refuse a
pair TOGETHER: a rank that refused on its local ranges while the other
went on would leave that one waiting in the combine's collective.  That
hang is the bug the refusal case exists for; the 120 s timeout turns it
into a failure.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_groupkeys_worker import AGGS, make_shard
from plan_minmax_ref import NULL_KEY, canon, eval_plan

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_groupkeys_worker.py")


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
    return run_world(2, tmp_path_factory.mktemp("gk_mp"))


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


def test_world2_ranges_are_agreed(results):
    n, data, nulls, shards = concat("agree")
    k0 = [s[0][0][2] for s in shards]
    assert (k0[0].min(), k0[0].max()) == (0, 49)
    assert (k0[1].min(), k0[1].max()) == (-40, 1039)
    assert not set(k0[0].tolist()) & set(k0[1].tolist())

    exp = canon(eval_plan(n, data, nulls, [], [], ["k0", "k1"], AGGS))
    exp12 = canon(eval_plan(n, data, nulls, [], [], ["k1", "k2"], AGGS))

    # pairs on both ranks and pairs on one rank only, in both plans
    def pairs(rank, cols):
        lo, hi = rank * (n // 2), (rank + 1) * (n // 2)
        return {tuple(NULL_KEY if nulls[c][i] else int(data[c][i])
                      for c in cols) for i in range(lo, hi)}
    for cols in (["k0", "k1"], ["k1", "k2"]):
        p0, p1 = pairs(0, cols), pairs(1, cols)
        assert p0 & p1 and p0 - p1 and p1 - p0

    for r in results:
        assert r["agree"] == exp
        assert r["agree_repeat"] == exp
        assert r["agree_after"] == exp
        assert r["agree12"] == exp12
        assert r["agree12_repeat"] == exp12
        assert "path_plan_group_packed" in r["paths"], r["paths"]


def test_world2_refuses_together(results):
    from greengage_amd import plan_group_bits
    _n, _data, _nulls, shards = concat("refuse")
    ranges = [[(int(s[0][g][2].min()), int(s[0][g][2].max()))
               for g in range(2)] for s in shards]
    # each rank's own ranges fit the budget, their union does not
    for (a0, b0), (a1, b1) in ranges:
        assert plan_group_bits([a0, a1], [b0, b1]) == (0, (31, 31))
    mn = [min(r[g][0] for r in ranges) for g in range(2)]
    mx = [max(r[g][1] for r in ranges) for g in range(2)]
    assert plan_group_bits(mn, mx) == (5, (32, 31))

    for r in results:
        assert r["refuse_error"] is not None, "the over-budget pair ran"
        assert "status 5:" in r["refuse_error"], r["refuse_error"]
        assert "32 + 31 bits" in r["refuse_error"], r["refuse_error"]
