#!/usr/bin/env python3
"""Cost of per-aggregate FILTER predicates on the compiled-plan path
(sibling of plan_payload_bench.py), synthetic TPC-H tables at --sf
(default 100).

Descriptors:
  q1      the unchanged Q1-shaped descriptor of plan_bench.py: no filter,
          so it must cost what it cost before filters existed.  Measured
          on the baked, generic (GG_PLAN_BAKE=0) and interpreted
          (GG_PLAN_RTC=0) tiers; the control against the parent commit.
  q1f     the same descriptor with SUM(price) and SUM(price*(100-disc))
          under FILTER (disc in [5, 8)) and COUNT(*) under FILTER
          (qty < 25.00): two filters on columns the plan loads anyway.
          Same tiers; compare against q1 of the same process.
  pivot   revenue per order year in ONE scan: lineitem INNER JOIN orders,
          no group column, four SUM(price*(100-disc)) each under FILTER
          (o_orderdate in one calendar year, 1993..1996) plus the
          unfiltered total.
  year    what plan_payload_bench.py measures for the same question:
          group by a host-derived year column of a copy of orders.
  pivot4  what a caller had to do before: four plans, each one
          SUM(price*(100-disc)) with the year range among the join's
          build predicates, so four scans of lineitem.  Reported per plan
          and as the sum of the four medians.

--warmup executes are excluded, then --reps executes are timed one by
one from the plan_scan_agg stat row (device-side events) and reported as
median [min .. max] in microseconds, with the build time per execute and
the path rows that ran.  One JSON line per measurement.

--pkg-root measures another checkout of the package (e.g. the parent
commit, built) with this same script; a checkout that predates filters
runs only q1, year and pivot4 (--only q1,year,pivot4).  To compare two
builds, run them interleaved as separate processes in one session and
compare the spread of the per-process medians.
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
ap.add_argument("--only", default="q1,q1f,pivot,year,pivot4")
ap.add_argument("--tiers", default="baked,generic,interp")
ap.add_argument("--pkg-root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()

sys.path.insert(0, args.pkg_root)
from greengage_amd import Engine, PGDate  # noqa: E402

NEG_INF = -(1 << 63)
only = args.only.split(",")
YEARS = [1993, 1994, 1995, 1996]


def year_range(y):
    return PGDate(f"{y}-01-01") + 0, PGDate(f"{y + 1}-01-01") + 0


def filt(agg, preds):
    return ("filter", agg, preds)


REV = ("sum", [("price", "id"), ("disc", "sub100")])
Q1 = ["count", ("sum", [("qty", "id")]), ("sum", [("price", "id")]),
      ("sum", [("disc", "id")]), REV,
      ("sum", [("price", "id"), ("disc", "sub100"), ("tax", "add100")])]
F_DISC = [("disc", 5, 8)]
Q1F = [filt("count", [("qty", NEG_INF, 2500)]), Q1[1],
       filt(Q1[2], F_DISC), Q1[3], filt(Q1[4], F_DISC), Q1[5]]

eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
rows = eng.table_nrows(li)
od = oy = None
if set(only) & {"pivot", "year", "pivot4"}:
    od = eng.register_synth("orders", seed=42, sf=args.sf)
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


def orders_join(table, preds=()):
    return [{"table": table, "build_key": "orderkey",
             "probe_key": "orderkey", "kind": "inner",
             "preds": list(preds)}]


def compile_desc(name):
    if name in ("q1", "q1f"):
        return eng.compile_plan(
            li, preds=[("shipdate", NEG_INF, PGDate("1998-08-15") + 1)],
            group_cols=["rflag", "lstatus"], aggs=Q1 if name == "q1" else Q1F)
    if name == "pivot":
        return eng.compile_plan(
            li, joins=orders_join(od),
            aggs=[filt(REV, [((0, "orderdate"),) + year_range(y)])
                  for y in YEARS] + [REV])
    if name == "year":
        return eng.compile_plan(li, joins=orders_join(oy),
                                group_cols=[(0, "oyear")],
                                aggs=[REV, "count"])
    assert name.startswith("pivot4_"), name
    return eng.compile_plan(
        li, joins=orders_join(
            od, [("orderdate",) + year_range(int(name[7:]))]), aggs=[REV])


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
    return res


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
        b0, _bl0 = stat(p, "plan_build")
        us = timed(p, lambda: eng.execute_plan(p, max_groups=64),
                   "plan_scan_agg")
        b1, _bl1 = stat(p, "plan_build")
    finally:
        os.environ.pop("GG_PLAN_BAKE", None)
        os.environ.pop("GG_PLAN_RTC", None)
    return first, report(name, tier, p, us, {
        "groups": len(first),
        "build_us_per_execute": round((b1 - b0) * 1000.0 / args.reps, 1)})


results = {}
for name in only:
    if name == "pivot4":
        # ungrouped plans are never baked: one tier
        per = [measure(f"pivot4_{y}", "generic") for y in YEARS]
        results["pivot4"] = [first[0][2][0] for first, _r in per]
        print(json.dumps({
            "tag": args.tag, "desc": "pivot4", "tier": "sum of 4 plans",
            "sf": args.sf, "rows": rows,
            "median_us": round(sum(r["median_us"] for _f, r in per), 1),
            "build_us_per_execute": round(
                sum(r["build_us_per_execute"] for _f, r in per), 1)}),
            flush=True)
        continue
    for tier in (args.tiers.split(",") if name in ("q1", "q1f", "year")
                 else ["generic", "interp"]):
        first, _r = measure(name, tier)
        if name == "pivot":
            results["pivot"] = first[0][2][:4]
# the one-scan pivot and the four separate plans answer the same question
if "pivot" in results and "pivot4" in results:
    assert results["pivot"] == results["pivot4"], results
eng.shutdown()
print("PLAN_FILTER_BENCH_OK")
