"""Multi-rank worker for MIN/MAX/AVG plans (one process per rank,
shared GPU, shm transport — see mp_engine_worker.py).

Each rank registers its OWN 20,000-row shard, so the only place the
ranks' MIN/MAX words, sums and counts meet is exec_plan's cross-segment
combine.  make_shard() is also what the test uses to rebuild both
shards for the reference.

Usage: python tests/mp_plan_minmax_worker.py RANK WORLD IDFILE OUTFILE
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NROWS = 20_000
AGGS = [("min", ("v", "id")), ("max", ("v", "id")),
        ("avg", [("v", "id")]), ("sum", [("w", "id"), ("v", "sub100")]),
        "count"]


def make_shard(rank):
    """Value ranges differ by rank: rank 0 holds the global MIN, rank 1
    the global MAX.  Group key 5 exists on rank 1 only; group 2 is
    all-NULL on rank 0 (and live on rank 1)."""
    rng = np.random.default_rng(1000 + rank)
    k = rng.integers(0, 5 + rank, NROWS).astype(np.int64)
    if rank == 0:
        v = rng.integers(-900_000, -1000, NROWS).astype(np.int64)
    else:
        v = rng.integers(-500, 700_000, NROWS).astype(np.int64)
    w = rng.integers(-120, 120, NROWS).astype(np.int64)
    vnull = rng.random(NROWS) < 0.1
    if rank == 0:
        vnull |= k == 2
    cols = [("k", "int64", k), ("v", "int64", v), ("w", "dec64", w)]
    return cols, {"v": vnull}


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
    t = eng.register_table("mm_shard", cols, NROWS)
    for c, nl in nullmap.items():
        eng.set_nulls(t, c, nl.astype(np.uint8))

    out = {"rank": rank}
    pg = eng.compile_plan(t, preds=[("w", -100, 110)], group_cols=["k"],
                          aggs=AGGS)
    out["grouped"] = eng.execute_plan(pg, max_groups=64)
    # the repeat takes the baked kernel (codes from the MERGED set)
    out["grouped_repeat"] = eng.execute_plan(pg, max_groups=64)
    p0 = eng.compile_plan(t, preds=[("w", -100, 110)], aggs=AGGS)
    out["global"] = eng.execute_plan(p0, max_groups=8)
    out["global_repeat"] = eng.execute_plan(p0, max_groups=8)
    out["paths"] = sorted(s["name"] for s in eng.stats(pg)
                          if s["name"].startswith("path"))

    eng.shutdown()
    with open(outfile + ".tmp", "w") as f:
        json.dump(out, f)
    os.rename(outfile + ".tmp", outfile)


if __name__ == "__main__":
    main()
