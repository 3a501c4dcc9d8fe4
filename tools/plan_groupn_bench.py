#!/usr/bin/env python3
"""Cost of three group columns on the compiled-plan path (sibling of
plan_payload_bench.py, same protocol), synthetic TPC-H tables at --sf
(default 100).

Descriptors, all over lineitem with `shipdate > 1995-03-15`, INNER JOIN
orders with `orderdate < 1995-03-15` (payload: custkey, orderdate,
shippriority), SEMI JOIN customer on the orders row's custkey with the
mktsegment predicate, SUM(price*(100-disc)), ORDER BY that sum DESC, the
order date ASC where it is a group column, LIMIT 10, est_groups = the rows
of orders:
  q3d     TPC-H Q3 as a descriptor: grouped by (orderkey, o_orderdate,
          o_shippriority), three packed fields (path_plan_group_packed_n)
  q3k2    grouped by (orderkey, o_orderdate): the packed pair
  q3k1    grouped by orderkey alone: the SAME groups as q3d (an order has
          one date and one priority), no payload group column, and the raw
          key as the code
  q3p1    grouped by the ORDERS row's orderkey alone: q3k1's groups, codes
          and hashes to the bit, but the key is a payload column, gathered
          at the build row like q3k2's and q3d's date: what separates the
          cost of a payload group column from the cost of a wide code
  q3      the named Q3 pipeline (GG_PIPE_Q3), whose dense maps and Bloom
          front the plan path does not have
  fold    no timing, a count: over every order with `orderdate < cutoff` (a
          superset of the plan's groups), how many DISTINCT 32-bit words
          gg_hashint8's xor-fold leaves of the q3d codes and of the raw
          order keys, and how many distinct start slots their hashes name in
          the plan's table.  Two codes that fold to one word share a start
          slot whatever the table's size; the raw keys are the yardstick

--warmup executes are excluded, then --reps executes are timed one by one:
`scan` from the plan_scan_agg stat row (device-side events), `build` from the
plan_build row, `wall` around the whole execute on the host clock, which is
the figure to hold against the named pipeline's.  Each is reported as median
[min .. max] in microseconds, with the path rows that ran and the number of
groups (the compacted rows the top-k selected from).  One JSON line per
measurement.

--pkg-root measures another checkout of the package with this same script.
To compare two builds, run them interleaved as separate processes in one
session and compare the spread of the per-process medians.
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=100)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--only", default="q3d,q3k2,q3k1,q3p1,q3,fold")
ap.add_argument("--tiers", default="generic,interp")
ap.add_argument("--pkg-root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()

sys.path.insert(0, args.pkg_root)
from greengage_amd import Engine, PGDate  # noqa: E402
from greengage_amd.engine import NEG_INF, PIPE_Q3, POS_INF  # noqa: E402

only = args.only.split(",")
CUTOFF = PGDate("1995-03-15")
GROUPS = {"q3d": ["orderkey", (0, "orderdate"), (0, "shippriority")],
          "q3k2": ["orderkey", (0, "orderdate")], "q3k1": ["orderkey"],
          "q3p1": [(0, "orderkey")]}

eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
od = eng.register_synth("orders", seed=42, sf=args.sf)
cu = eng.register_synth("customer", seed=42, sf=args.sf)
rows = eng.table_nrows(li)


def compile_desc(name):
    cols = GROUPS[name]
    return eng.compile_plan(
        li, preds=[("shipdate", CUTOFF + 1, POS_INF)],
        joins=[{"table": od, "build_key": "orderkey", "probe_key": "orderkey",
                "kind": "inner", "preds": [("orderdate", NEG_INF, CUTOFF)]},
               {"table": cu, "build_key": "custkey", "probe_key": "custkey",
                "kind": "semi", "probe_src": 1, "preds": [("mktseg", 2, 3)]}],
        group_cols=cols,
        aggs=[("sum", [("price", "id"), ("disc", "sub100")])],
        order_by=[("agg", 0, "desc")] +
        ([("key", 1, "asc")] if len(cols) > 1 else []),
        limit=10, est_groups=eng.table_nrows(od))


def stat(p, name, field="total_ms"):
    for s in eng.stats(p):
        if s["name"] == name:
            return s[field], s["launches"]
    return 0.0, 0


def spread(us):
    return {"median_us": round(statistics.median(us), 1),
            "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def timed(p, execute, stat_rows):
    """per-execute microseconds of each stat row, and of the whole execute on
    the host clock, over --reps executes"""
    out = {r: [] for r in stat_rows}
    wall = []
    for _ in range(args.reps):
        before = {r: stat(p, r)[0] for r in stat_rows}
        t0 = time.perf_counter()
        execute()
        wall.append((time.perf_counter() - t0) * 1e6)
        for r in stat_rows:
            out[r].append((stat(p, r)[0] - before[r]) * 1000.0)
    return out, wall


def report(name, tier, p, per_row, wall, extra):
    res = {"tag": args.tag, "desc": name, "tier": tier, "sf": args.sf,
           "rows": rows, "warmup": args.warmup, "reps": args.reps,
           "wall": spread(wall),
           "paths": sorted(s["name"] for s in eng.stats(p)
                           if s["name"].startswith("path"))}
    for r, us in per_row.items():
        res[r] = spread(us)
    res.update(extra)
    print(json.dumps(res), flush=True)


def measure(name, tier):
    if tier == "interp":
        os.environ["GG_PLAN_RTC"] = "0"
    try:
        p = compile_desc(name)
        first = eng.execute_plan_keys(p)
        # the top-k's candidates of one execute: every group
        groups = int(stat(p, "plan_topk", "rows_in")[0])
        for _ in range(args.warmup):
            assert eng.execute_plan_keys(p) == first
        per_row, wall = timed(p, lambda: eng.execute_plan_keys(p),
                              ["plan_scan_agg", "plan_build", "plan_topk"])
    finally:
        os.environ.pop("GG_PLAN_RTC", None)
    report(name, tier, p, per_row, wall, {
        "groups": groups,
        "top": [[list(k), v] for k, v in first[:2]]})


def fold_report():
    import numpy as np
    from greengage_amd import plan_group_bits_n
    cols = [eng.fetch_column(od, c, t).astype(np.int64)
            for c, t in (("orderkey", np.int64), ("orderdate", np.int32),
                         ("shippriority", np.int32))]
    mins = [int(c.min()) for c in cols]
    rc, bits = plan_group_bits_n(mins, [int(c.max()) for c in cols])
    assert rc == 0, bits
    keep = cols[1] < CUTOFF
    code = np.zeros(int(keep.sum()), np.uint64)
    for c, mn, b in zip(cols, mins, bits):
        code = (code << np.uint64(b)) | (c[keep] - mn + 1).astype(np.uint64)
    # the plan's table: next_pow2(2 * est_groups), est_groups = orders rows
    nslots = 1
    while nslots < 2 * len(cols[0]):
        nslots <<= 1

    def hash_u32(k):
        # gg_hash_uint32: Jenkins final() over the seeded lanes
        u = np.uint32
        rot = lambda x, r: (x << u(r)) | (x >> u(32 - r))  # noqa: E731
        a = b = c = u((0x9e3779b9 + 4 + 3923095) & 0xffffffff)
        a = a + k
        b = np.full_like(k, b)
        c = np.full_like(k, c)
        for x, y, r in ((2, 1, 14), (0, 2, 11), (1, 0, 25), (2, 1, 16),
                        (0, 2, 4), (1, 0, 14), (2, 1, 24)):
            v = [a, b, c]
            v[x] = (v[x] ^ v[y]) - rot(v[y], r)
            a, b, c = v
        return c

    res = {"tag": args.tag, "desc": "fold", "sf": args.sf, "bits": list(bits),
           "codes": len(code), "nslots": nslots}
    for nm, w in (("q3d", code), ("q3k1", cols[0][keep].astype(np.uint64))):
        folded = (w & np.uint64(0xffffffff)) ^ (w >> np.uint64(32))
        folded = folded.astype(np.uint32)
        res[nm + "_distinct_folded"] = int(len(np.unique(folded)))
        slots = hash_u32(folded) & np.uint32(nslots - 1)
        res[nm + "_distinct_start_slots"] = int(len(np.unique(slots)))
    print(json.dumps(res), flush=True)


for name in only:
    if name == "fold":
        fold_report()
        continue
    if name == "q3":
        p3 = eng.compile(PIPE_Q3, lineitem=li, orders=od, customer=cu,
                         cutoff_date=CUTOFF, mktsegment=2, limit_k=10)
        for _ in range(1 + args.warmup):
            top, hdr = eng.execute_q3(p3)
        names = [s["name"] for s in eng.stats(p3)
                 if not s["name"].startswith("path")]
        per_row, wall = timed(p3, lambda: eng.execute_q3(p3), names)
        report("q3", "named", p3, per_row, wall, {
            "groups": hdr["n_groups"], "join_rows": hdr["n_join_rows"],
            "top": [[r["orderkey"], r["revenue4"]] for r in top[:2]]})
        continue
    for tier in args.tiers.split(","):
        measure(name, tier)
eng.shutdown()
print("PLAN_GROUPN_BENCH_OK")
