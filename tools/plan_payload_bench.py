#!/usr/bin/env python3
"""Cost of INNER joins with payload columns on the compiled-plan path
(sibling of plan_minmax_bench.py), synthetic TPC-H tables at --sf
(default 100).

Descriptors:
  q1      the unchanged Q1-shaped descriptor of plan_bench.py: no join,
          so it must cost what it cost before payload joins existed.
          Measured on the baked, generic (GG_PLAN_BAKE=0) and interpreted
          (GG_PLAN_RTC=0) tiers.
  q1i32   the same descriptor over a copy of lineitem whose rflag and
          lstatus are registered as int32 instead of char1: the pair is
          then no (char1, char1) pair and takes the packed group code
          (path_plan_group_packed).  Same rows, same groups, same tiers;
          the two group columns are 4 bytes wide instead of 1.
  year    revenue by order year: lineitem INNER JOIN orders on orderkey
          (dense index map), SUM(price*(100-disc)) and COUNT(*) grouped
          by a payload column.  The year is derived on the host from
          o_orderdate and registered beside o_orderkey as table
          `orders_y`; descriptors cannot compute expressions.
  nation  the three-table chain: lineitem -> orders (payload custkey)
          -> customer, COUNT(*) grouped by c_nationkey.
  q3      the named Q3 pipeline, for orientation: its probe_lineitem
          stat row probes the same lineitem -> orders join.

--warmup executes are excluded, then --reps executes are timed one by
one from the plan_scan_agg stat row (device-side events; probe_lineitem
for q3) and reported as median [min .. max] in microseconds, with the
build time per execute and the path rows that ran.  One JSON line per
measurement.

--pkg-root measures another checkout of the package (e.g. the parent
commit, built) with this same script; a checkout that predates payload
joins runs only `q1` (--only q1).  To compare two builds, run them
interleaved as separate processes in one session and compare the
spread of the per-process medians.
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=100)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--only", default="q1,q1i32,year,nation,q3")
ap.add_argument("--tiers", default="baked,generic,interp")
ap.add_argument("--pkg-root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()

sys.path.insert(0, args.pkg_root)
from greengage_amd import Engine, PGDate  # noqa: E402
from greengage_amd.engine import PIPE_Q3  # noqa: E402

NEG_INF = -(1 << 63)
only = args.only.split(",")

Q1 = ["count", ("sum", [("qty", "id")]), ("sum", [("price", "id")]),
      ("sum", [("disc", "id")]),
      ("sum", [("price", "id"), ("disc", "sub100")]),
      ("sum", [("price", "id"), ("disc", "sub100"), ("tax", "add100")])]

eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
rows = eng.table_nrows(li)
od = cu = oy = li32 = None
if "q1i32" in only:
    import numpy as np
    li32 = eng.register_table(
        "lineitem_g32",
        [(c, ty, eng.fetch_column(li, c, dt).astype(dt2, copy=False))
         for c, ty, dt, dt2 in (
             [("shipdate", "int32", np.int32, np.int32)] +
             [(c, "dec64", np.int64, np.int64)
              for c in ("qty", "price", "disc", "tax")] +
             [(c, "int32", np.uint8, np.int32)
              for c in ("rflag", "lstatus")])], rows)
if set(only) & {"year", "nation", "q3"}:
    od = eng.register_synth("orders", seed=42, sf=args.sf)
    cu = eng.register_synth("customer", seed=42, sf=args.sf)
if "year" in only:
    import numpy as np
    days = eng.fetch_column(od, "orderdate", np.int32)
    year = ((np.datetime64("2000-01-01") + days.astype("timedelta64[D]"))
            .astype("datetime64[Y]").astype(np.int64) + 1970)
    oy = eng.register_table(
        "orders_y", [("orderkey", "int64",
                      eng.fetch_column(od, "orderkey", np.int64)),
                     ("oyear", "int32", year.astype(np.int32))], len(days))
    del days, year


def compile_desc(name):
    if name in ("q1", "q1i32"):
        return eng.compile_plan(
            li if name == "q1" else li32,
            preds=[("shipdate", NEG_INF, PGDate("1998-08-15") + 1)],
            group_cols=["rflag", "lstatus"], aggs=Q1)
    if name == "year":
        return eng.compile_plan(
            li, joins=[{"table": oy, "build_key": "orderkey",
                        "probe_key": "orderkey", "kind": "inner"}],
            group_cols=[(0, "oyear")],
            aggs=[("sum", [("price", "id"), ("disc", "sub100")]), "count"])
    assert name == "nation", name
    return eng.compile_plan(
        li, joins=[{"table": od, "build_key": "orderkey",
                    "probe_key": "orderkey", "kind": "inner"},
                   {"table": cu, "build_key": "custkey",
                    "probe_key": "custkey", "kind": "inner",
                    "probe_src": 1}],
        group_cols=[(1, "nationkey")], aggs=["count"])


def stat(p, name):
    for s in eng.stats(p):
        if s["name"] == name:
            return s["total_ms"], s["launches"]
    return 0.0, 0


def timed(p, execute, row):
    """per-execute microseconds of stat row `row` over --reps executes"""
    us = []
    for _ in range(args.reps):
        t0, l0 = stat(p, row)
        execute()
        t1, l1 = stat(p, row)
        assert l1 == l0 + 1
        us.append((t1 - t0) * 1000.0)
    return us


def report(name, tier, p, us, extra):
    res = {"tag": args.tag, "desc": name, "tier": tier, "sf": args.sf,
           "rows": rows, "warmup": args.warmup, "reps": args.reps,
           "median_us": round(statistics.median(us), 1),
           "min_us": round(min(us), 1), "max_us": round(max(us), 1),
           "paths": sorted(s["name"] for s in eng.stats(p)
                           if s["name"].startswith("path"))}
    res.update(extra)
    print(json.dumps(res), flush=True)


def measure(name, tier):
    if tier == "generic":
        os.environ["GG_PLAN_BAKE"] = "0"
    elif tier == "interp":
        os.environ["GG_PLAN_RTC"] = "0"
    try:
        p = compile_desc(name)
        first = eng.execute_plan(p, max_groups=64)
        for _ in range(args.warmup):
            assert eng.execute_plan(p, max_groups=64) == first
        b0, bl0 = stat(p, "plan_build")
        us = timed(p, lambda: eng.execute_plan(p, max_groups=64),
                   "plan_scan_agg")
        b1, bl1 = stat(p, "plan_build")
    finally:
        os.environ.pop("GG_PLAN_BAKE", None)
        os.environ.pop("GG_PLAN_RTC", None)
    report(name, tier, p, us, {
        "groups": len(first),
        "build_us_per_execute": round((b1 - b0) * 1000.0 / args.reps, 1)})


for name in only:
    if name == "q3":
        p3 = eng.compile(PIPE_Q3, lineitem=li, orders=od, customer=cu,
                         cutoff_date=PGDate("1995-03-15"), mktsegment=2,
                         limit_k=10)
        for _ in range(1 + args.warmup):
            eng.execute_q3(p3)
        report("q3", "named", p3,
               timed(p3, lambda: eng.execute_q3(p3), "probe_lineitem"),
               {"row": "probe_lineitem"})
        continue
    for tier in args.tiers.split(","):
        measure(name, tier)
eng.shutdown()
print("PLAN_PAYLOAD_BENCH_OK")
