#!/usr/bin/env python3
"""Cost of LEFT OUTER and ANTI joins on the compiled-plan path (sibling of
plan_filter_bench.py), synthetic TPC-H tables at --sf (default 100).

Descriptors, ONE per process (--desc):
  q1              the unchanged Q1-shaped descriptor of plan_bench.py: no
                  join.  Control against the parent commit.
  year            revenue per order year: lineitem INNER JOIN a copy of
                  orders carrying a host-derived year column, grouped by
                  it.  Unchanged plan, the second control.
  year_left       `year` with the join made LEFT.  Every lineitem row has
                  its order, so no row is NULL-extended and the result is
                  `year`'s: what the partner flag costs when it never
                  fires.  Compare against the PARENT's `year`.
  year_left_half  the same with the ON-clause oyear < 1995, which removes
                  about half of the build rows: those lineitem rows are
                  NULL-extended into the NULL group.
  noorder_anti    lineitem ANTI JOIN the same build side under the same
                  predicate (NOT EXISTS an order before 1995), COUNT(*).

--warmup executes are excluded, then --reps executes are timed one by one
from the plan_scan_agg stat row (device-side events) and reported as median
[min .. max] in microseconds per tier (baked, generic = GG_PLAN_BAKE=0,
interp = GG_PLAN_RTC=0), with the build time per execute and the path rows
that ran.  One JSON line per measurement.

--pkg-root measures another checkout of the package (the parent commit,
built) with this same script; it knows only q1 and year.

--drive is the session: for --rounds rounds it starts, one process after
the other, the branch and then the parent for each control, then the
branch for each new descriptor, so that branch and parent runs interleave
and the parent-versus-parent spread of the same session is on record.  It
then prints the ratios.  The driver itself never opens the GPU.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCS = ["q1", "year", "year_left", "year_left_half", "noorder_anti"]
CONTROLS = ["q1", "year"]

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=100)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--desc", default="year_left", choices=DESCS)
ap.add_argument("--tiers", default="baked,generic,interp")
ap.add_argument("--pkg-root", default=HERE)
ap.add_argument("--tag", default="")
ap.add_argument("--drive", action="store_true")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--parent-root", default="",
                help="--drive: a built checkout of the parent commit")
args = ap.parse_args()


def drive():
    results = []

    def child(tag, desc, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--desc", desc,
               "--tag", tag, "--sf", str(args.sf), "--warmup",
               str(args.warmup), "--reps", str(args.reps), "--tiers",
               args.tiers, "--pkg-root", root]
        print(f"== plan_outer_bench.py --desc {desc} --tag {tag}", flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=600)
        text = r.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if r.returncode != 0:
            # a failed child ends the session: nothing more is started
            sys.exit(f"{tag} {desc}: rc={r.returncode}")
        results.extend(json.loads(ln) for ln in text.splitlines()
                       if ln.startswith("{"))

    for rnd in range(1, args.rounds + 1):
        for desc in CONTROLS:
            child(f"branch-{rnd}", desc, HERE)
            if args.parent_root:
                child(f"parent-{rnd}", desc, args.parent_root)
        for desc in DESCS:
            if desc not in CONTROLS:
                child(f"branch-{rnd}", desc, HERE)

    def med(side, desc, tier):
        return [r["median_us"] for r in results
                if r["tag"].startswith(side) and r["desc"] == desc
                and r["tier"] == tier]

    for tier in args.tiers.split(","):
        summary = {"summary": tier}
        for desc in CONTROLS:
            b, p = med("branch", desc, tier), med("parent", desc, tier)
            if b and p:
                summary[f"{desc}_branch_over_parent"] = round(
                    statistics.median(b) / statistics.median(p), 4)
                summary[f"{desc}_parent_spread"] = round(
                    (max(p) - min(p)) / statistics.median(p), 4)
                summary[f"{desc}_branch_spread"] = round(
                    (max(b) - min(b)) / statistics.median(b), 4)
        base = med("parent", "year", tier) or med("branch", "year", tier)
        for desc in ("year_left", "year_left_half", "noorder_anti"):
            b = med("branch", desc, tier)
            if b and base:
                summary[f"{desc}_over_parent_year"] = round(
                    statistics.median(b) / statistics.median(base), 4)
        print(json.dumps(summary), flush=True)
    print("PLAN_OUTER_BENCH_OK")


if args.drive:
    drive()
    sys.exit(0)

sys.path.insert(0, args.pkg_root)
from greengage_amd import Engine, PGDate  # noqa: E402

NEG_INF = -(1 << 63)
REV = ("sum", [("price", "id"), ("disc", "sub100")])
Q1 = ["count", ("sum", [("qty", "id")]), ("sum", [("price", "id")]),
      ("sum", [("disc", "id")]), REV,
      ("sum", [("price", "id"), ("disc", "sub100"), ("tax", "add100")])]
HALF = [("oyear", NEG_INF, 1995)]

eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
rows = eng.table_nrows(li)
oy = None
if args.desc != "q1":
    import numpy as np
    od = eng.register_synth("orders", seed=42, sf=args.sf)
    days = eng.fetch_column(od, "orderdate", np.int32)
    year = ((np.datetime64("2000-01-01") + days.astype("timedelta64[D]"))
            .astype("datetime64[Y]").astype(np.int64) + 1970)
    oy = eng.register_table(
        "orders_y", [("orderkey", "int64",
                      eng.fetch_column(od, "orderkey", np.int64)),
                     ("oyear", "int32", year.astype(np.int32))], len(days))
    del days, year


def orders_join(kind, preds=()):
    return [{"table": oy, "build_key": "orderkey", "probe_key": "orderkey",
             "kind": kind, "preds": list(preds)}]


def compile_desc(name):
    if name == "q1":
        return eng.compile_plan(
            li, preds=[("shipdate", NEG_INF, PGDate("1998-08-15") + 1)],
            group_cols=["rflag", "lstatus"], aggs=Q1)
    if name == "noorder_anti":
        return eng.compile_plan(li, joins=orders_join("anti", HALF),
                                aggs=["count"])
    kind, preds = {"year": ("inner", ()), "year_left": ("left", ()),
                   "year_left_half": ("left", HALF)}[name]
    return eng.compile_plan(li, joins=orders_join(kind, preds),
                            group_cols=[(0, "oyear")], aggs=[REV, "count"])


def stat(p, name):
    for s in eng.stats(p):
        if s["name"] == name:
            return s["total_ms"], s["launches"]
    return 0.0, 0


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
        b0, _l = stat(p, "plan_build")
        us = []
        for _ in range(args.reps):
            t0, l0 = stat(p, "plan_scan_agg")
            eng.execute_plan(p, max_groups=64)
            t1, l1 = stat(p, "plan_scan_agg")
            assert l1 == l0 + 1
            us.append((t1 - t0) * 1000.0)
        b1, _l = stat(p, "plan_build")
    finally:
        os.environ.pop("GG_PLAN_BAKE", None)
        os.environ.pop("GG_PLAN_RTC", None)
    print(json.dumps({
        "tag": args.tag, "desc": name, "tier": tier, "sf": args.sf,
        "rows": rows, "warmup": args.warmup, "reps": args.reps,
        "median_us": round(statistics.median(us), 1),
        "min_us": round(min(us), 1), "max_us": round(max(us), 1),
        "paths": sorted(s["name"] for s in eng.stats(p)
                        if s["name"].startswith("path")),
        "groups": len(first),
        # COUNT(*) over all groups: first aggregate of q1 and of
        # noorder_anti, second of the year plans
        "rows_counted": sum(
            g[2][0 if name in ("q1", "noorder_anti") else 1] for g in first),
        "build_us_per_execute": round((b1 - b0) * 1000.0 / args.reps, 1)}),
        flush=True)
    return first


# ungrouped plans are never baked: one generated tier
tiers = [t for t in args.tiers.split(",")
         if not (args.desc == "noorder_anti" and t == "baked")]
firsts = [measure(args.desc, t) for t in tiers]
assert all(f == firsts[0] for f in firsts), "tiers disagree"
eng.shutdown()
