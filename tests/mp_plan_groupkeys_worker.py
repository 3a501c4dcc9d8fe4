"""Multi-rank worker for packed two-column group keys (one process per
rank, shared GPU, shm transport — see mp_plan_minmax_worker.py).

Each rank registers its OWN shard.  The packed code is built from the
columns' value ranges, so the ranks must agree on the ranges before any
of them packs: their codes meet in exec_plan's cross-segment combine.
make_shard() is also what the test uses to rebuild both shards for the
reference.

Table `agree`: the ranks' k0 ranges are disjoint — rank 0 holds [0, 50),
rank 1 [-40, 0) and [1000, 1040) — so a (k0, k1) pair lives on both
ranks only through a NULL k0 (both columns are nullable); k1 is [0, 9)
on rank 0 and [3, 10) on rank 1, k2 [0, 4) and [2, 6), so the (k1, k2)
pairs mix: some on both ranks, some on one.
Table `refuse`: each rank's own k0 range takes 31 bits, as k1 does, so
either rank alone would accept the pair; the union of the k0 ranges
takes 32 and both ranks must refuse.

Usage: python tests/mp_plan_groupkeys_worker.py RANK WORLD IDFILE OUTFILE
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
EDGE = (1 << 31) - 2


def make_shard(rank):
    """{table: (cols, nullmap)}"""
    rng = np.random.default_rng(3000 + rank)
    if rank == 0:
        k0 = rng.integers(0, 50, NROWS)
        k1 = rng.integers(0, 9, NROWS)
        k2 = rng.integers(0, 4, NROWS)
    else:
        k0 = np.where(rng.random(NROWS) < 0.5,
                      rng.integers(-40, 0, NROWS),
                      rng.integers(1000, 1040, NROWS))
        k1 = rng.integers(3, 10, NROWS)
        k2 = rng.integers(2, 6, NROWS)
    v = rng.integers(-1000, 100_000, NROWS)
    agree = ([("k0", "int64", k0.astype(np.int64)),
              ("k1", "int32", k1.astype(np.int32)),
              ("k2", "int64", k2.astype(np.int64)),
              ("v", "int64", v.astype(np.int64))],
             {"k0": rng.random(NROWS) < 0.1, "k1": rng.random(NROWS) < 0.1})
    r0 = rng.choice([0, EDGE] if rank == 0
                    else [1 << 31, (1 << 32) - 2], 101)
    r1 = rng.choice([0, EDGE], 101)
    r0[:2] = [0, EDGE] if rank == 0 else [1 << 31, (1 << 32) - 2]
    r1[:2] = [0, EDGE]
    refuse = ([("k0", "int64", r0.astype(np.int64)),
               ("k1", "int64", r1.astype(np.int64)),
               ("v", "int64", v[:101].astype(np.int64))], {})
    return {"agree": agree, "refuse": refuse}


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
        tabs[name] = eng.register_table(f"gk_{name}", cols, len(cols[0][2]))
        for c, nl in nullmap.items():
            eng.set_nulls(tabs[name], c, nl.astype(np.uint8))

    out = {"rank": rank}
    pa = eng.compile_plan(tabs["agree"], group_cols=["k0", "k1"], aggs=AGGS)
    out["agree"] = eng.execute_plan(pa, max_groups=2048)
    out["agree_repeat"] = eng.execute_plan(pa, max_groups=2048)
    pb = eng.compile_plan(tabs["agree"], group_cols=["k1", "k2"], aggs=AGGS)
    out["agree12"] = eng.execute_plan(pb, max_groups=2048)
    out["agree12_repeat"] = eng.execute_plan(pb, max_groups=2048)
    out["paths"] = sorted(s["name"] for s in eng.stats(pa)
                          if s["name"].startswith("path"))
    # every rank must refuse on the AGREED ranges; a rank deciding on
    # its own would sail on into the combine and wait there for ever
    try:
        pr = eng.compile_plan(tabs["refuse"], group_cols=["k0", "k1"],
                              aggs=AGGS)
        eng.execute_plan(pr, max_groups=16)
        out["refuse_error"] = None
    except EngineError as e:
        out["refuse_error"] = str(e)
    # and the engine goes on: the agreed plan still answers
    out["agree_after"] = eng.execute_plan(pa, max_groups=2048)

    eng.shutdown()
    with open(outfile + ".tmp", "w") as f:
        json.dump(out, f)
    os.rename(outfile + ".tmp", outfile)


if __name__ == "__main__":
    main()
