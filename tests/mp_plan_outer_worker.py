"""Multi-rank worker for LEFT OUTER and ANTI joins (one process per rank,
shared GPU, shm transport, see mp_plan_groupkeys_worker.py).

Each rank registers its OWN shard of the driving table and the whole
(replicated) build table.  Rank 0's shard holds only rows with a partner,
rank 1's only rows without one: the NULL group exists on rank 1 alone and
the payload groups on rank 0 alone, and both must come out of the
cross-segment combine on both ranks.  make_tables() is also what the test
uses to rebuild both shards for the reference.

Usage: python tests/mp_plan_outer_worker.py RANK WORLD IDFILE OUTFILE
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NROWS = 6001
MBUILD = 601
AGGS = ["count", ("count", (0, "w")), ("sum", [("x", "id"), ((0, "w"), "id")]),
        ("max", ((0, "w"), "id")), ("avg", [((0, "w"), "add100")])]
ANTI_AGGS = ["count", ("sum", [("x", "id")]), ("min", ("x", "id"))]
PLANS = {
    "left": dict(kind="left", group_cols=[(0, "c")], aggs=AGGS),
    # a packed pair with a LEFT payload column: ranges agreed across ranks
    "left_pair": dict(kind="left", group_cols=[(0, "s"), "g"], aggs=AGGS),
    "anti": dict(kind="anti", group_cols=["g"], aggs=ANTI_AGGS),
}


def make_tables(rank):
    """(build cols, build nullmap, driving cols, driving nullmap)"""
    rb = np.random.default_rng(4000)            # the same on every rank
    keys = (rb.permutation(np.arange(2 * MBUILD))[:MBUILD] + 1).astype(
        np.int64)
    bcols = [("bk", "int64", keys),
             ("w", "int32", rb.integers(-50, 50, MBUILD).astype(np.int32)),
             ("c", "char1", rb.integers(0, 3, MBUILD).astype(np.uint8)),
             ("s", "int32", rb.integers(-2, 2, MBUILD).astype(np.int32))]
    bnull = {"w": rb.random(MBUILD) < 0.2}
    rng = np.random.default_rng(4001 + rank)
    absent = np.concatenate([
        np.setdiff1d(np.arange(1, 2 * MBUILD + 1), keys),
        [-3, 0, 2 * MBUILD + 9, 1 << 40]])
    fk = rng.choice(keys if rank == 0 else absent, NROWS)
    dcols = [("x", "int32", rng.integers(-100, 100, NROWS).astype(np.int32)),
             ("g", "int64", rng.integers(rank, rank + 3, NROWS).astype(
                 np.int64)),
             ("fk", "int64", fk.astype(np.int64))]
    return bcols, bnull, dcols, {}


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

    bcols, bnull, dcols, dnull = make_tables(rank)
    bt = eng.register_table("po_build", bcols, MBUILD)
    for c, nl in bnull.items():
        eng.set_nulls(bt, c, nl.astype(np.uint8))
    dt = eng.register_table("po_drive", dcols, NROWS)
    for c, nl in dnull.items():
        eng.set_nulls(dt, c, nl.astype(np.uint8))

    out = {"rank": rank, "paths": {}}
    for name, spec in PLANS.items():
        p = eng.compile_plan(
            dt, joins=[{"table": bt, "build_key": "bk", "probe_key": "fk",
                        "kind": spec["kind"]}],
            group_cols=spec["group_cols"], aggs=spec["aggs"])
        out[name] = [eng.execute_plan(p, max_groups=256) for _ in range(3)]
        out["paths"][name] = sorted(s["name"] for s in eng.stats(p)
                                    if s["name"].startswith("path"))

    eng.shutdown()
    with open(outfile + ".tmp", "w") as f:
        json.dump(out, f)
    os.rename(outfile + ".tmp", outfile)


if __name__ == "__main__":
    main()
