"""Multi-rank worker for three packed group columns (one process per rank,
shared GPU, shm transport: see mp_plan_groupkeys_worker.py, whose protocol
this follows).

Each rank registers its OWN shard.  The code of a G = 3 plan is built from the
value ranges of all three columns, agreed across the ranks in one allgather
before any of them packs.  make_shard() is also what the test uses to rebuild
both shards for the reference.

Table `agree`: k0 is [0, 5) on rank 0 and [3, 8) on rank 1 (nullable on
both), k1 [0, 3) on both; the third column k2 is [0, 4) on rank 0 and [2, 6)
or [1000, 1003) on rank 1, so its local width is 3 bits on rank 0 and its
agreed width 10: a rank packing on its own range would shift k0 and k1 to
other bit positions than its peer.  Groups with k2 in {2, 3} live on both
ranks.
Table `refuse`: k0 takes 31 bits and k1 30 on either rank; k2 is the single
value 0 on rank 0 and 1 on rank 1, one bit locally (31 + 30 + 1 = 62, either
rank alone would accept) and two bits agreed: both ranks must refuse.

Usage: python tests/mp_plan_groupn_worker.py RANK WORLD IDFILE OUTFILE
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NROWS = 10_007
AGGS = ["count", ("sum", [("v", "id")]), ("max", ("v", "id")),
        ("avg", [("v", "id")])]
COLS = ["k0", "k1", "k2"]
E31 = (1 << 31) - 2
E30 = (1 << 30) - 2


def make_shard(rank):
    """{table: (cols, nullmap)}"""
    rng = np.random.default_rng(4100 + rank)
    if rank == 0:
        k0 = rng.integers(0, 5, NROWS)
        k2 = rng.integers(0, 4, NROWS)
    else:
        k0 = rng.integers(3, 8, NROWS)
        k2 = np.where(rng.random(NROWS) < 0.6, rng.integers(2, 6, NROWS),
                      rng.integers(1000, 1003, NROWS))
    k1 = rng.integers(0, 3, NROWS)
    v = rng.integers(-1000, 100_000, NROWS)
    agree = ([("k0", "int64", k0.astype(np.int64)),
              ("k1", "int32", k1.astype(np.int32)),
              ("k2", "int64", k2.astype(np.int64)),
              ("v", "int64", v.astype(np.int64))],
             {"k0": rng.random(NROWS) < 0.1})
    r0 = rng.choice([0, E31], 101)
    r1 = rng.choice([0, E30], 101)
    r0[:2] = [0, E31]
    r1[:2] = [0, E30]
    refuse = ([("k0", "int64", r0.astype(np.int64)),
               ("k1", "int64", r1.astype(np.int64)),
               ("k2", "int32", np.full(101, rank, np.int32)),
               ("v", "int64", v[:101].astype(np.int64))], {})
    return {"agree": agree, "refuse": refuse}


def rows(groups):
    """execute_plan_keys output in a form that survives JSON"""
    return [[list(k), [list(v) if isinstance(v, tuple) else v for v in vals]]
            for k, vals in groups]


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    idfile, outfile = sys.argv[3], sys.argv[4]

    from greengage_amd import Engine, EngineError

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

    tabs = {}
    for name, (cols, nullmap) in make_shard(rank).items():
        tabs[name] = eng.register_table(f"gn_{name}", cols, len(cols[0][2]))
        for c, nl in nullmap.items():
            eng.set_nulls(tabs[name], c, nl.astype(np.uint8))

    out = {"rank": rank}
    pa = eng.compile_plan(tabs["agree"], group_cols=COLS, aggs=AGGS)
    out["agree"] = rows(eng.execute_plan_keys(pa, max_groups=2048))
    out["agree_repeat"] = rows(eng.execute_plan_keys(pa, max_groups=2048))
    out["paths"] = sorted(s["name"] for s in eng.stats(pa)
                          if s["name"].startswith("path"))
    # every rank must refuse on the AGREED ranges; a rank deciding on its
    # own would go on into the combine and wait there for its peer
    out["refuse_errors"] = []
    pr = eng.compile_plan(tabs["refuse"], group_cols=COLS, aggs=AGGS)
    for _ in range(2):
        try:
            eng.execute_plan_keys(pr, max_groups=16)
            out["refuse_errors"].append(None)
        except EngineError as e:
            out["refuse_errors"].append(str(e))
    # and the engine goes on: the agreed plan still answers
    out["agree_after"] = rows(eng.execute_plan_keys(pa, max_groups=2048))

    eng.shutdown()
    with open(outfile + ".tmp", "w") as f:
        json.dump(out, f)
    os.rename(outfile + ".tmp", outfile)


if __name__ == "__main__":
    main()
