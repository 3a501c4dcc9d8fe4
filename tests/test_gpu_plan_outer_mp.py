"""LEFT OUTER and ANTI joins at world 2 on ONE GPU over the shm transport,
launched like test_gpu_plan_groupkeys_mp.py launches its worker.

Segment 0's shard holds only rows with a partner, segment 1's only rows
without one.  The NULL group therefore comes from one segment and the
payload groups from the other, the ANTI plan's survivors all from segment
1, and the packed pair's ranges must still be agreed: every rank reports
the evaluator's result over the concatenated shards, on all three
executes.  Two processes only.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mp_plan_outer_worker import MBUILD, NROWS, PLANS, make_tables
from plan_minmax_ref import canon
from plan_outer_ref import NULL_KEY, eval_plan

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "mp_plan_outer_worker.py")


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
    return run_world(2, tmp_path_factory.mktemp("po_mp"))


def _evaluator_form(cols, nullmap):
    n = len(cols[0][2])
    data = {c: np.asarray(a).astype(np.int64) for c, _t, a in cols}
    nulls = {c: np.asarray(nullmap.get(c, np.zeros(n, bool))).astype(bool)
             for c in data}
    return data, nulls


@pytest.fixture(scope="module")
def expected():
    shards = [make_tables(r) for r in range(2)]
    bdata, bnulls = _evaluator_form(shards[0][0], shards[0][1])
    dcols = [(c, t, np.concatenate([s[2][i][2] for s in shards]))
             for i, (c, t, _a) in enumerate(shards[0][2])]
    data, nulls = _evaluator_form(dcols, {})
    exp = {}
    for name, spec in PLANS.items():
        joins = [{"build_key": "bk", "probe_key": "fk", "kind": spec["kind"],
                  "_data": bdata, "_nulls": bnulls, "_n": MBUILD}]
        exp[name] = eval_plan(2 * NROWS, data, nulls, [], joins,
                              spec["group_cols"], spec["aggs"])
    return exp


def test_world2_left_join(results, expected):
    exp = expected["left"]
    # the NULL group is segment 1's rows, the rest segment 0's
    assert exp[0][0] == NULL_KEY and exp[0][2][0] == NROWS
    assert sum(v[0] for _a, _b, v in exp[1:]) == NROWS and len(exp) == 4
    for r in results:
        for got in r["left"]:
            assert got == canon(exp)
        assert "path_plan_join_left" in r["paths"]["left"]
        assert "path_plan_join_anti" not in r["paths"]["left"]


def test_world2_left_join_packed_pair(results, expected):
    exp = expected["left_pair"]
    assert sum(k0 == NULL_KEY for k0, _k1, _v in exp) == 3
    for r in results:
        for got in r["left_pair"]:
            assert got == canon(exp)
        assert "path_plan_group_packed" in r["paths"]["left_pair"]


def test_world2_anti_join(results, expected):
    exp = expected["anti"]
    assert sum(v[0] for _a, _b, v in exp) == NROWS
    assert [k0 for k0, _k1, _v in exp] == [1, 2, 3]
    for r in results:
        for got in r["anti"]:
            assert got == canon(exp)
        assert "path_plan_join_anti" in r["paths"]["anti"]
        assert "path_plan_join_left" not in r["paths"]["anti"]
