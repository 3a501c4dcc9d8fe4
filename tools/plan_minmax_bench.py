#!/usr/bin/env python3
"""Cost of MIN/MAX/AVG on the compiled-plan path (sibling of
plan_bench.py), lineitem at --sf (default 100, as plan_bench.py).

Descriptors, all grouped by (rflag, lstatus) under the Q1 cutoff:
  q1    the unchanged Q1-shaped descriptor of plan_bench.py (6 aggs)
  base  count, sum(price*(100-disc))
  mm    base + MIN(qty), MAX(price), AVG(disc)
The Q1-shaped descriptor already holds 6 aggregates, so adding three
more exceeds GG_PLAN_MAX_AGGS (8) before any lowering; `base`/`mm` is
the largest Q1-shaped pair that fits: mm lowers to exactly 8
accumulator slots and reads only columns q1 already streams.

Each descriptor is measured on the baked tier (default) and on the
generic RTC tier (GG_PLAN_BAKE=0); --tiers can add `interp`, the
interpreted fallback kernel (GG_PLAN_RTC=0).  --warmup executes are
excluded, then --reps executes are timed one by one from the
plan_scan_agg stat row (device-side events) and reported as median
[min .. max] in microseconds.
One JSON line per measurement.

--pkg-root measures another checkout of the package (e.g. the parent
commit, built) with this same script; such a checkout may predate the
new kinds, so only `q1` runs there (--only q1).
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
ap.add_argument("--only", default="q1,base,mm")
ap.add_argument("--tiers", default="baked,generic")
ap.add_argument("--pkg-root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()

sys.path.insert(0, args.pkg_root)
from greengage_amd import Engine, PGDate  # noqa: E402

NEG_INF = -(1 << 63)

Q1 = ["count", ("sum", [("qty", "id")]), ("sum", [("price", "id")]),
      ("sum", [("disc", "id")]),
      ("sum", [("price", "id"), ("disc", "sub100")]),
      ("sum", [("price", "id"), ("disc", "sub100"), ("tax", "add100")])]
BASE = ["count", ("sum", [("price", "id"), ("disc", "sub100")])]
MM = BASE + [("min", ("qty", "id")), ("max", ("price", "id")),
             ("avg", [("disc", "id")])]
DESCS = {"q1": Q1, "base": BASE, "mm": MM}

eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
rows = eng.table_nrows(li)
cutoff = PGDate("1998-08-15")


def scan_ms(p):
    for s in eng.stats(p):
        if s["name"] == "plan_scan_agg":
            return s["total_ms"], s["launches"]
    return 0.0, 0


def measure(name, tier):
    if tier == "generic":
        os.environ["GG_PLAN_BAKE"] = "0"
    elif tier == "interp":
        os.environ["GG_PLAN_RTC"] = "0"
    try:
        p = eng.compile_plan(
            li, preds=[("shipdate", NEG_INF, cutoff + 1)],
            group_cols=["rflag", "lstatus"], aggs=DESCS[name])
        first = eng.execute_plan(p, max_groups=16)
        for _ in range(args.warmup):
            assert eng.execute_plan(p, max_groups=16) == first
        us = []
        for _ in range(args.reps):
            t0, l0 = scan_ms(p)
            eng.execute_plan(p, max_groups=16)
            t1, l1 = scan_ms(p)
            assert l1 == l0 + 1
            us.append((t1 - t0) * 1000.0)
    finally:
        os.environ.pop("GG_PLAN_BAKE", None)
        os.environ.pop("GG_PLAN_RTC", None)
    paths = sorted(s["name"] for s in eng.stats(p)
                   if s["name"].startswith("path"))
    res = {"tag": args.tag, "desc": name, "tier": tier, "sf": args.sf,
           "rows": rows, "warmup": args.warmup, "reps": args.reps,
           "median_us": round(statistics.median(us), 1),
           "min_us": round(min(us), 1), "max_us": round(max(us), 1),
           "paths": paths}
    print(json.dumps(res), flush=True)
    return res


out = {}
for name in args.only.split(","):
    for tier in args.tiers.split(","):
        out[(name, tier)] = measure(name, tier)
for tier in args.tiers.split(","):
    if ("mm", tier) in out and ("base", tier) in out:
        r = out[("mm", tier)]["median_us"] / out[("base", tier)]["median_us"]
        q = out[("mm", tier)]["median_us"] / out[("q1", tier)]["median_us"] \
            if ("q1", tier) in out else float("nan")
        print(f"ratio {tier}: mm/base = {r:.3f}, mm/q1 = {q:.3f}")
eng.shutdown()
print("PLAN_MINMAX_BENCH_OK")
