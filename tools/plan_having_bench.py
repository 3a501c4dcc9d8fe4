#!/usr/bin/env python3
"""Cost of HAVING on the compiled-plan path (sibling of plan_order_bench.py
and plan_where_bench.py).

The shape is TPC-H Q18's inner block over the synthetic lineitem at --sf:
    SELECT l_orderkey, SUM(l_quantity) FROM lineitem GROUP BY l_orderkey
    HAVING SUM(l_quantity) > 300 ORDER BY SUM(l_quantity) DESC LIMIT 100
with est_groups = the orders table's rows (1.5M x sf groups, of which a few
in a hundred thousand pass).

Descriptors, ONE per process (--desc):
  device    the plan with its HAVING: selected on the device, the top 100 of
            the survivors copied out.
  host      the same plan under GG_PLAN_HAVING=host: every group copied out,
            filtered and partially sorted on the host.
  baseline  what the parent commit offers: the plan WITHOUT HAVING, order or
            limit (a limit above an undone HAVING would give wrong rows), so
            every group lands in the arena in key order, and the caller
            filters the arena and takes the top 100 (numpy over the arena
            here, which is kind to the baseline).  It checks its rows against
            nothing; --drive compares the three results.

Timing.  Wall time of gg_engine_execute into a preallocated arena, plus the
caller's filter for `baseline`, with the plan_scan_agg, plan_having and
plan_topk stat rows (device events) beside it.  --warmup executes are
excluded, --reps are timed one by one: median [min .. max] in microseconds.
One JSON line per measurement.

--drive is the session: it starts the three descriptors one process after
the other, checks that all three report the same rows, and prints the
ratios.  The driver itself never opens the GPU.
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
DESCS = ["device", "host", "baseline"]

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=10)
ap.add_argument("--threshold", type=int, default=300,
                help="HAVING SUM(l_quantity) > this, in whole units")
ap.add_argument("--limit", type=int, default=100)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--desc", default="device", choices=DESCS)
ap.add_argument("--tag", default="")
ap.add_argument("--drive", action="store_true")
args = ap.parse_args()


def drive():
    results = []
    for desc in DESCS:
        cmd = [sys.executable, os.path.abspath(__file__), "--desc", desc,
               "--tag", args.tag or "branch", "--sf", str(args.sf),
               "--threshold", str(args.threshold), "--limit",
               str(args.limit), "--warmup", str(args.warmup), "--reps",
               str(args.reps)]
        print(f"== plan_having_bench.py --desc {desc}", flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=900)
        text = r.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if r.returncode != 0:
            # a failed child ends the session: nothing more is started
            sys.exit(f"{desc}: rc={r.returncode}")
        results.extend(json.loads(ln) for ln in text.splitlines()
                       if ln.startswith("{"))
    by = {r["desc"]: r for r in results}
    assert len({r["rows_sha1"] for r in results}) == 1, \
        "the three forms disagree on the result"
    summary = {"summary": "median wall time per execute, us", "sf": args.sf,
               "groups": by["device"]["groups"],
               "survivors": by["device"]["survivors"]}
    for d in DESCS:
        summary[d] = by[d]["median_us"]
    summary["device_over_baseline"] = round(
        by["device"]["median_us"] / by["baseline"]["median_us"], 4)
    summary["host_over_baseline"] = round(
        by["host"]["median_us"] / by["baseline"]["median_us"], 4)
    print(json.dumps(summary), flush=True)
    print("PLAN_HAVING_BENCH_OK")


if args.drive:
    drive()
    sys.exit(0)

sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
from greengage_amd import Engine  # noqa: E402
from greengage_amd import engine as ge  # noqa: E402

name = args.desc
# l_quantity is a scale-2 decimal: the caller applies the scale
bound = args.threshold * 100
eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
od = eng.register_synth("orders", seed=42, sf=args.sf)
rows, est = eng.table_nrows(li), eng.table_nrows(od)
aggs = [("sum", [("qty", "id")])]
if name == "baseline":
    p = eng.compile_plan(li, group_cols=["orderkey"], aggs=aggs,
                         est_groups=est)
    max_rows = est
else:
    p = eng.compile_plan(li, group_cols=["orderkey"], aggs=aggs,
                         est_groups=est, order_by=[("agg", 0, "desc")],
                         limit=args.limit, having=[("cmp", 0, ">", bound)])
    max_rows = args.limit
if name == "host":
    os.environ["GG_PLAN_HAVING"] = "host"

ROW = 4                         # int64 words per arena row: k0, k1, lo, hi
arena_bytes = 16 + max_rows * ROW * 8
arena = ctypes.create_string_buffer(arena_bytes)
written = ctypes.c_size_t()


def execute():
    """(wall us, the result rows as an int64 array of (key, sum))"""
    t0 = time.perf_counter()
    rc = ge.lib().gg_engine_execute(p, arena, arena_bytes,
                                    ctypes.byref(written))
    assert rc == 0, ge.lib().gg_engine_last_error()
    n = int.from_bytes(arena[0:8], "little", signed=True)
    a = np.frombuffer(arena, np.int64, n * ROW, 16).reshape(n, ROW)
    if name == "baseline":
        # the caller's HAVING, ORDER BY and LIMIT; the sums fit int64
        # (hi is the sign word), the total order is (sum desc, key asc)
        a = a[a[:, 2] > bound]
        a = a[np.lexsort((a[:, 0], -a[:, 2]))][:args.limit]
    out = a[:, [0, 2]].copy()
    return (time.perf_counter() - t0) * 1e6, out


def stat(row, field="total_ms"):
    for s in eng.stats(p):
        if s["name"] == row:
            return s[field]
    return 0


first_us, head = execute()      # compiles the generated kernel
for _ in range(args.warmup):
    execute()
wall, dev = [], {"plan_scan_agg": [], "plan_having": [], "plan_topk": []}
for _ in range(args.reps):
    before = {k: stat(k) for k in dev}
    us, out = execute()
    wall.append(us)
    for k in dev:
        dev[k].append((stat(k) - before[k]) * 1000.0)
    assert np.array_equal(out, head), "result changed between executes"
execs = 1 + args.warmup + args.reps
print(json.dumps({
    "tag": args.tag, "desc": name, "sf": args.sf, "rows": rows,
    "groups": (stat("plan_having", "rows_in") // execs) or None,
    "survivors": (stat("plan_having", "rows_out") // execs
                  if name == "device" else None),
    "rows_out": len(head),
    "rows_sha1": hashlib.sha1(head.tobytes()).hexdigest(),
    "warmup": args.warmup, "reps": args.reps,
    "median_us": round(statistics.median(wall), 1),
    "min_us": round(min(wall), 1), "max_us": round(max(wall), 1),
    "scan_us": round(statistics.median(dev["plan_scan_agg"]), 1),
    "having_us": round(statistics.median(dev["plan_having"]), 1),
    "topk_us": round(statistics.median(dev["plan_topk"]), 1),
    "first_execute_us": round(first_us, 1),
    "paths": {s["name"]: s["launches"] for s in eng.stats(p)
              if s["name"].startswith("path")}}), flush=True)
eng.shutdown()
