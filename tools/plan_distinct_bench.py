#!/usr/bin/env python3
"""Cost of COUNT(DISTINCT) on the compiled-plan path (sibling of
plan_having_bench.py).

Two plans over the synthetic tables at --sf, ONE plan and path per process:
  nation    distinct customers per nation: few groups, millions of pairs
              SELECT c_nationkey, COUNT(DISTINCT o_custkey), COUNT(*)
              FROM orders JOIN customer ON o_custkey = c_custkey
              GROUP BY c_nationkey
            (25 groups; one (nation, customer) pair per customer that has an
            order; est_groups = the customer table's rows)
  customer  distinct order dates per customer: a high-cardinality group column
              SELECT o_custkey, COUNT(DISTINCT o_orderdate), COUNT(*)
              FROM orders GROUP BY o_custkey
              ORDER BY COUNT(DISTINCT o_orderdate) DESC LIMIT 100
            (a group per customer that has an order, nearly a pair per order;
            est_groups = the orders table's rows)
  --path device   the regroup on the device (the default path)
  --path host     the same plan under GG_PLAN_DISTINCT=host: every pair copied
                  out and folded on the host

Timing.  Wall time of gg_engine_execute into a preallocated arena, with the
plan_scan_agg and plan_regroup stat rows beside it (device events; the host
path books no time on plan_regroup).  --warmup executes are excluded, --reps
are timed one by one: median [min .. max] in microseconds.  One JSON line per
measurement.

--drive is the session: it starts the four combinations one process after the
other, checks that the two paths of a plan report the same rows, and prints
the ratios.  The driver itself never opens the GPU.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = ["nation", "customer"]
PATHS = ["device", "host"]

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=100)
ap.add_argument("--plan", default="nation", choices=PLANS)
ap.add_argument("--path", default="device", choices=PATHS)
ap.add_argument("--limit", type=int, default=100)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--tag", default="")
ap.add_argument("--drive", action="store_true")
args = ap.parse_args()


def drive():
    results = []
    for plan in PLANS:
        for path in PATHS:
            cmd = [sys.executable, os.path.abspath(__file__), "--plan", plan,
                   "--path", path, "--tag", args.tag or "branch", "--sf",
                   str(args.sf), "--limit", str(args.limit), "--warmup",
                   str(args.warmup), "--reps", str(args.reps)]
            print(f"== plan_distinct_bench.py --plan {plan} --path {path}",
                  flush=True)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=900)
            text = r.stdout.decode()
            sys.stdout.write(text)
            sys.stdout.flush()
            if r.returncode != 0:
                # a failed child ends the session: nothing more is started
                sys.exit(f"{plan}/{path}: rc={r.returncode}")
            results.extend(json.loads(ln) for ln in text.splitlines()
                           if ln.startswith("{"))
    by = {(r["plan"], r["path"]): r for r in results}
    summary = {"summary": "median wall time per execute, us", "sf": args.sf}
    for plan in PLANS:
        d, h = by[plan, "device"], by[plan, "host"]
        assert d["rows_sha1"] == h["rows_sha1"], \
            f"{plan}: the two paths disagree on the result"
        summary[plan] = {"pairs": d["pairs"], "groups": d["groups"],
                         "device": d["median_us"], "host": h["median_us"],
                         "device_over_host": round(
                             d["median_us"] / h["median_us"], 4)}
    print(json.dumps(summary), flush=True)
    print("PLAN_DISTINCT_BENCH_OK")


if args.drive:
    drive()
    sys.exit(0)

sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
from greengage_amd import Engine  # noqa: E402
from greengage_amd import engine as ge  # noqa: E402

if args.path == "host":
    os.environ["GG_PLAN_DISTINCT"] = "host"
eng = Engine(device=0, n_segments=1, segment_id=0)
od = eng.register_synth("orders", seed=42, sf=args.sf)
rows = eng.table_nrows(od)
aggs = [("count_distinct", "custkey" if args.plan == "nation"
         else "orderdate"), "count"]
if args.plan == "nation":
    cu = eng.register_synth("customer", seed=42, sf=args.sf)
    p = eng.compile_plan(
        od, joins=[{"table": cu, "build_key": "custkey",
                    "probe_key": "custkey", "kind": "inner"}],
        group_cols=[(0, "nationkey")], aggs=aggs,
        est_groups=eng.table_nrows(cu))
    max_rows = 256
else:
    p = eng.compile_plan(od, group_cols=["custkey"], aggs=aggs,
                         est_groups=rows,
                         order_by=[("agg", 0, "desc")], limit=args.limit)
    max_rows = args.limit

ROW = 2 + 2 * len(aggs)         # int64 words per arena row
arena_bytes = 16 + max_rows * ROW * 8
arena = ctypes.create_string_buffer(arena_bytes)
written = ctypes.c_size_t()


def execute():
    """(wall us, the result rows as an int64 array)"""
    t0 = time.perf_counter()
    rc = ge.lib().gg_engine_execute(p, arena, arena_bytes,
                                    ctypes.byref(written))
    assert rc == 0, ge.lib().gg_engine_last_error()
    us = (time.perf_counter() - t0) * 1e6
    n = int.from_bytes(arena[0:8], "little", signed=True)
    return us, np.frombuffer(arena, np.int64, n * ROW, 16).reshape(
        n, ROW).copy()


def stat(row, field="total_ms"):
    for s in eng.stats(p):
        if s["name"] == row:
            return s[field]
    return 0


first_us, head = execute()      # compiles the generated kernel
for _ in range(args.warmup):
    execute()
wall, dev = [], {"plan_scan_agg": [], "plan_regroup": []}
for _ in range(args.reps):
    before = {k: stat(k) for k in dev}
    us, out = execute()
    wall.append(us)
    for k in dev:
        dev[k].append((stat(k) - before[k]) * 1000.0)
    assert np.array_equal(out, head), "result changed between executes"
execs = 1 + args.warmup + args.reps


def spread(v):
    return [round(statistics.median(v), 1), round(min(v), 1),
            round(max(v), 1)]


print(json.dumps({
    "tag": args.tag, "plan": args.plan, "path": args.path, "sf": args.sf,
    "rows": rows,
    "pairs": stat("plan_regroup", "rows_in") // execs,
    "groups": stat("plan_regroup", "rows_out") // execs,
    "rows_out": len(head),
    "rows_sha1": hashlib.sha1(head.tobytes()).hexdigest(),
    "warmup": args.warmup, "reps": args.reps,
    "median_us": round(statistics.median(wall), 1),
    "min_us": round(min(wall), 1), "max_us": round(max(wall), 1),
    "scan_us_med_min_max": spread(dev["plan_scan_agg"]),
    "regroup_us_med_min_max": spread(dev["plan_regroup"]),
    "first_execute_us": round(first_us, 1),
    "paths": {s["name"]: s["launches"] for s in eng.stats(p)
              if s["name"].startswith("path")}}), flush=True)
eng.shutdown()
