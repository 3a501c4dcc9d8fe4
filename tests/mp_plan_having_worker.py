"""Multi-rank worker for HAVING (one process per rank, shared GPU, shm
transport, see mp_plan_order_worker.py).

Each rank registers its OWN shard of the driving table.  Every group has
two rows on each rank, and the groups come in four classes by their SUM(x)
against the plans' HAVING SUM(x) > 300:
  0  about 200 on each rank: passes only after the cross-segment combine
  1  about 350 on rank 0 and -100 on rank 1: passes on rank 0 alone, fails
     combined
  2  about 400 on each rank: passes everywhere
  3  about 10 on each rank: fails everywhere
so a HAVING evaluated per segment, ahead of the combine, would be wrong both
ways (test_gpu_plan_having_mp.py asserts that of the shards).  make_shard()
is also what the test uses to rebuild both shards for the reference.

Usage: python tests/mp_plan_having_worker.py RANK WORLD IDFILE OUTFILE
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NGROUPS = 200
NROWS = 2 * NGROUPS
AGGS = [("sum", [("x", "id")]), "count", ("max", ("m", "id"))]
SUM_GT_300 = ("cmp", 0, ">", 300)
PLANS = {
    # the survivors in key order
    "having": dict(having=[SUM_GT_300]),
    # the top groups among the survivors
    "having_top": dict(having=[SUM_GT_300], order_by=[("agg", 0, "desc")],
                       limit=10, est_groups=1000),
    # COUNT(*) is 2 on each rank: >= 4 holds only combined
    "having_count": dict(having=[("cmp", 1, ">=", 4),
                                 [("range", 0, 0, 300), ("is_null", 2)]],
                         order_by=[("agg", 0, "asc")]),
}
TARGET = {0: (200, 200), 1: (350, -100), 2: (400, 400), 3: (10, 10)}


def make_shard(rank):
    """(driving cols, nullmap) of one rank"""
    rng = np.random.default_rng(6600 + rank)
    g = np.arange(NGROUPS)
    total = np.array([TARGET[c][rank] for c in g % 4]) + rng.integers(
        -20, 20, NGROUPS)
    first = total // 2 + rng.integers(-30, 30, NGROUPS)
    k = np.concatenate([g, g])
    x = np.concatenate([first, total - first])
    perm = rng.permutation(NROWS)
    cols = [("k", "int64", (k[perm] * 11 - 500).astype(np.int64)),
            ("x", "int64", x[perm].astype(np.int64)),
            ("m", "int32", rng.integers(-40, 40, NROWS).astype(np.int32))]
    return cols, {"m": rng.random(NROWS) < 0.6}


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
    dt = eng.register_table("phav_drive", cols, NROWS)
    for c, nl in nullmap.items():
        eng.set_nulls(dt, c, nl.astype(np.uint8))

    out = {"rank": rank, "paths": {}}
    for name, spec in PLANS.items():
        p = eng.compile_plan(dt, group_cols=["k"], aggs=AGGS, **spec)
        out[name] = [eng.execute_plan(p, max_groups=512) for _ in range(3)]
        out["paths"][name] = sorted(s["name"] for s in eng.stats(p)
                                    if s["name"].startswith("path"))

    eng.shutdown()
    with open(outfile + ".tmp", "w") as f:
        json.dump(out, f)
    os.rename(outfile + ".tmp", outfile)


if __name__ == "__main__":
    main()
