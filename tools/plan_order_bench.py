#!/usr/bin/env python3
"""Cost of ORDER BY / LIMIT and of a grown group table on the compiled-plan
path (sibling of plan_outer_bench.py).

Descriptors, ONE per process (--desc):
  groups      SUM(x), COUNT(*) GROUP BY k over a host-built table of
              --groups groups (default 131,072, which the fixed group table
              holds) x --rows-per-group rows; unordered, every group copied
              out.  The parent commit runs it too: the baseline.
  top10       the same with ORDER BY SUM(x) DESC LIMIT 10: device top-k,
              10 rows copied out.
  top10_host  top10 under GG_PLAN_TOPK=host: every group copied out and
              partially sorted on the host.
  q1          the unchanged Q1-shaped descriptor of plan_bench.py over the
              synthetic lineitem at --sf: the control against the parent.
  orderkey    SUM(price), COUNT(*) GROUP BY orderkey over lineitem at --sf,
              ORDER BY SUM DESC LIMIT 10 with est_groups = the orders
              table's rows: 1.5M x sf groups, far past the fixed table.
              Reports scan, top-k and the rest of the execute separately.

Timing.  groups/top10/top10_host/orderkey: wall time of gg_engine_execute
into a preallocated arena (what the caller waits for: scan, compact, top-k
or copy-out, host ordering, arena), with the plan_scan_agg and plan_topk
stat rows (device events) beside it; `rest_us` is wall minus those two:
the compact kernel, the copy back and the host work.  q1: the
plan_scan_agg stat row per execute, as in plan_outer_bench.py.  --warmup
executes are excluded, --reps are timed one by one: median [min .. max] in
microseconds.  One JSON line per measurement.

--pkg-root measures another checkout of the package (the parent commit,
built) with this same script; it knows only `groups` and `q1`.

--drive is the session: for --rounds rounds it starts, one process after
the other, branch and parent for `groups` and `q1` and the branch for the
two top-10 forms, so that branch and parent runs interleave and the
run-to-run spread of each side is on record; then it prints the ratios.
The driver itself never opens the GPU.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCS = ["groups", "top10", "top10_host", "q1", "orderkey"]
BOTH = ["groups", "q1"]

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=10)
ap.add_argument("--groups", type=int, default=131072)
ap.add_argument("--rows-per-group", type=int, default=32)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--desc", default="top10", choices=DESCS)
ap.add_argument("--pkg-root", default=HERE)
ap.add_argument("--tag", default="")
ap.add_argument("--drive", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--parent-root", default="",
                help="--drive: a built checkout of the parent commit")
args = ap.parse_args()


def drive():
    results = []

    def child(tag, desc, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--desc", desc,
               "--tag", tag, "--sf", str(args.sf), "--groups",
               str(args.groups), "--rows-per-group",
               str(args.rows_per_group), "--warmup", str(args.warmup),
               "--reps", str(args.reps), "--pkg-root", root]
        print(f"== plan_order_bench.py --desc {desc} --tag {tag}", flush=True)
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
        for desc in BOTH:
            child(f"branch-{rnd}", desc, HERE)
            if args.parent_root:
                child(f"parent-{rnd}", desc, args.parent_root)
        for desc in ("top10", "top10_host"):
            child(f"branch-{rnd}", desc, HERE)

    def med(side, desc):
        return [r["median_us"] for r in results
                if r["tag"].startswith(side) and r["desc"] == desc]

    def spread(v):
        return round((max(v) - min(v)) / statistics.median(v), 4)

    summary = {"summary": "medians of the rounds' medians, us"}
    for desc in DESCS:
        for side in ("branch", "parent"):
            v = med(side, desc)
            if v:
                summary[f"{desc}_{side}"] = round(statistics.median(v), 1)
                summary[f"{desc}_{side}_spread"] = spread(v)
    for desc in BOTH:
        b, p = med("branch", desc), med("parent", desc)
        if b and p:
            summary[f"{desc}_branch_over_parent"] = round(
                statistics.median(b) / statistics.median(p), 4)
    base = med("parent", "groups") or med("branch", "groups")
    for desc in ("top10", "top10_host"):
        b = med("branch", desc)
        if b and base:
            summary[f"{desc}_over_unordered"] = round(
                statistics.median(b) / statistics.median(base), 4)
    print(json.dumps(summary), flush=True)
    print("PLAN_ORDER_BENCH_OK")


if args.drive:
    drive()
    sys.exit(0)

sys.path.insert(0, args.pkg_root)
import numpy as np  # noqa: E402
from greengage_amd import Engine, PGDate  # noqa: E402
from greengage_amd import engine as ge  # noqa: E402

NEG_INF = -(1 << 63)
Q1 = ["count", ("sum", [("qty", "id")]), ("sum", [("price", "id")]),
      ("sum", [("disc", "id")]),
      ("sum", [("price", "id"), ("disc", "sub100")]),
      ("sum", [("price", "id"), ("disc", "sub100"), ("tax", "add100")])]
TOP = dict(order_by=[("agg", 0, "desc")], limit=10)

eng = Engine(device=0, n_segments=1, segment_id=0)
name = args.desc
if name == "q1":
    li = eng.register_synth("lineitem", seed=42, sf=args.sf)
    rows = eng.table_nrows(li)
    p = eng.compile_plan(
        li, preds=[("shipdate", NEG_INF, PGDate("1998-08-15") + 1)],
        group_cols=["rflag", "lstatus"], aggs=Q1)
    max_rows = 8
elif name == "orderkey":
    li = eng.register_synth("lineitem", seed=42, sf=args.sf)
    od = eng.register_synth("orders", seed=42, sf=args.sf)
    rows = eng.table_nrows(li)
    p = eng.compile_plan(li, group_cols=["orderkey"],
                         aggs=[("sum", [("price", "id")]), "count"],
                         est_groups=eng.table_nrows(od), **TOP)
    max_rows = 10
else:
    rng = np.random.default_rng(7)
    rows = args.groups * args.rows_per_group
    k = (rng.permutation(rows) % args.groups).astype(np.int64) * 3 + 1
    x = rng.integers(-10 ** 6, 10 ** 6, rows).astype(np.int64)
    t = eng.register_table("pob", [("k", "int64", k), ("x", "int64", x)],
                           rows)
    p = eng.compile_plan(t, group_cols=["k"],
                         aggs=[("sum", [("x", "id")]), "count"],
                         **({} if name == "groups" else TOP))
    max_rows = args.groups if name != "top10" else 10
if name == "top10_host":
    os.environ["GG_PLAN_TOPK"] = "host"
    max_rows = 10

arena_bytes = 16 + max_rows * (16 + 16 * 8)
arena = ctypes.create_string_buffer(arena_bytes)
written = ctypes.c_size_t()


def execute():
    t0 = time.perf_counter()
    rc = ge.lib().gg_engine_execute(p, arena, arena_bytes,
                                    ctypes.byref(written))
    t1 = time.perf_counter()
    assert rc == 0, ge.lib().gg_engine_last_error()
    return (t1 - t0) * 1e6


def stat_ms(row):
    for s in eng.stats(p):
        if s["name"] == row:
            return s["total_ms"]
    return 0.0


first_us = execute()          # compiles the generated kernel; may regrow
n_groups = int.from_bytes(arena.raw[0:8], "little", signed=True)
head = arena.raw[16:16 + 48]
for _ in range(args.warmup):
    execute()
wall, scan, topk = [], [], []
for _ in range(args.reps):
    s0, k0 = stat_ms("plan_scan_agg"), stat_ms("plan_topk")
    wall.append(execute())
    scan.append((stat_ms("plan_scan_agg") - s0) * 1000.0)
    topk.append((stat_ms("plan_topk") - k0) * 1000.0)
assert arena.raw[16:16 + 48] == head, "result changed between executes"
us = scan if name == "q1" else wall
print(json.dumps({
    "tag": args.tag, "desc": name, "rows": rows, "groups_out": n_groups,
    "warmup": args.warmup, "reps": args.reps,
    "timed": "plan_scan_agg" if name == "q1" else "wall",
    "median_us": round(statistics.median(us), 1),
    "min_us": round(min(us), 1), "max_us": round(max(us), 1),
    "scan_us": round(statistics.median(scan), 1),
    "topk_us": round(statistics.median(topk), 1),
    "rest_us": round(statistics.median(
        [w - s - k for w, s, k in zip(wall, scan, topk)]), 1),
    "first_execute_us": round(first_us, 1),
    # groups the top-k chose from, and its tournament rounds per execute
    "topk_groups_in": next((s["rows_in"] // (1 + args.warmup + args.reps)
                            for s in eng.stats(p)
                            if s["name"] == "plan_topk"), 0),
    "topk_rounds": next((s["launches"] // (1 + args.warmup + args.reps)
                         for s in eng.stats(p)
                         if s["name"] == "plan_topk"), 0),
    "paths": {s["name"]: s["launches"] for s in eng.stats(p)
              if s["name"].startswith("path")}}), flush=True)
eng.shutdown()
