"""Multi-rank worker for COUNT(DISTINCT) (one process per rank, shared GPU,
shm transport, see mp_plan_order_worker.py).

Each rank registers its OWN shard of the driving table.  Every group has rows
on both ranks, and within a group some values of x occur on both ranks, some
on one only: a distinct count per segment, added up, would count the shared
values twice (test_gpu_plan_distinct_mp.py asserts that of the shards).  The
(group key, value) pairs are combined across the segments by their inner
code, which counts a shared value once, and regrouped on the host.
make_shard() is also what the test uses to rebuild both shards for the
reference.

Usage: python tests/mp_plan_distinct_worker.py RANK WORLD IDFILE OUTFILE
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NGROUPS = 40
NROWS = 1200
CDX = ("count_distinct", "x")
AGGS = [CDX, "count", ("filter", CDX, [("f", 0, 2)]), ("max", ("x", "id"))]
PLANS = {
    # the groups in key order
    "groups": dict(group_cols=["k"]),
    # one global group
    "global": dict(group_cols=[]),
    # the top groups by distinct count among those a HAVING keeps
    "top": dict(group_cols=["k"], having=[("cmp", 0, ">=", 36)],
                order_by=[("agg", 0, "desc")], limit=7, est_groups=4000),
}


def make_shard(rank):
    """(driving cols, nullmap) of one rank: x is drawn from 30 values both
    ranks share and 15 that only this rank has"""
    rng = np.random.default_rng(7400 + rank)
    shared = np.arange(30) * 7 - 100
    own = 1000 * (rank + 1) + np.arange(15)
    cols = [("k", "int64", (rng.integers(0, NGROUPS, NROWS) * 13 - 200).astype(
                np.int64)),
            ("x", "int64", rng.choice(np.concatenate([shared, own]),
                                      NROWS).astype(np.int64)),
            ("f", "int64", rng.integers(0, 4, NROWS).astype(np.int64))]
    return cols, {"x": rng.random(NROWS) < 0.1, "k": rng.random(NROWS) < 0.03}


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    idfile, outfile = sys.argv[3], sys.argv[4]

    from greengage_amd import Engine

    eng = Engine(device=0, n_segments=world, segment_id=rank)
    if rank == 0:
        cid = eng.comm_id()
        assert cid.startswith(b"GGSHM:"), "worker requires GG_COMM_SHM=1"
        with open(idfile + ".tmp", "wb") as f:
            f.write(cid)
        os.rename(idfile + ".tmp", idfile)
    else:
        for _ in range(600):
            if os.path.exists(idfile):
                break
            time.sleep(0.1)
        with open(idfile, "rb") as f:
            cid = f.read()
    eng.comm_init(cid)

    cols, nullmap = make_shard(rank)
    dt = eng.register_table("pdist_drive", cols, NROWS)
    for c, nl in nullmap.items():
        eng.set_nulls(dt, c, nl.astype(np.uint8))

    out = {"rank": rank, "paths": {}, "regroup": {}}
    for name, spec in PLANS.items():
        p = eng.compile_plan(dt, aggs=AGGS, **spec)
        out[name] = [eng.execute_plan(p, max_groups=512) for _ in range(3)]
        st = {s["name"]: s for s in eng.stats(p)}
        out["paths"][name] = sorted(s for s in st if s.startswith("path"))
        out["regroup"][name] = [st["plan_regroup"]["launches"],
                                st["plan_regroup"]["rows_in"],
                                st["plan_regroup"]["rows_out"]]

    eng.shutdown()
    with open(outfile + ".tmp", "w") as f:
        json.dump(out, f)
    os.rename(outfile + ".tmp", outfile)


if __name__ == "__main__":
    main()
