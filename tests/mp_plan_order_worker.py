"""Multi-rank worker for ORDER BY / LIMIT (one process per rank, shared GPU,
shm transport, see mp_plan_outer_worker.py).

Each rank registers its OWN shard of the driving table.  Every group has
rows on both ranks, with unrelated values on each, so a group's SUM and MAX
exist only after the cross-segment combine and neither rank's local top-10
is the global one (test_gpu_plan_order_mp.py asserts that of the shards).
make_shard() is also what the test uses to rebuild both shards for the
reference.

Usage: python tests/mp_plan_order_worker.py RANK WORLD IDFILE OUTFILE
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NGROUPS = 400
NROWS = 1000
AGGS = [("sum", [("x", "id")]), "count", ("max", ("m", "id"))]
PLANS = {
    # top-k by an aggregate no segment knows alone
    "top": dict(order_by=[("agg", 0, "desc")], limit=10, est_groups=0),
    "bottom_max": dict(order_by=[("agg", 2, "asc", "nulls_first"),
                                 ("agg", 1, "desc")], limit=60,
                       est_groups=1000),
    # an order without a limit: every group, ordered
    "all": dict(order_by=[("agg", 1, "desc"), ("agg", 0, "asc")], limit=0,
                est_groups=0),
    # a limit alone: the key order, cut
    "keys": dict(order_by=[], limit=7, est_groups=0),
}


def make_shard(rank):
    """(driving cols, nullmap) of one rank"""
    rng = np.random.default_rng(6000 + rank)
    k = np.concatenate([np.arange(NGROUPS),
                        rng.integers(0, NGROUPS, NROWS - NGROUPS)])
    cols = [("k", "int64", (k * 11 - 500).astype(np.int64)),
            ("x", "int64", rng.integers(0, 1000, NROWS).astype(np.int64)),
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
    dt = eng.register_table("pord_drive", cols, NROWS)
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
