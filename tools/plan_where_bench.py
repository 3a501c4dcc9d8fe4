#!/usr/bin/env python3
"""Cost of general WHERE clauses on the compiled-plan path (sibling of
plan_outer_bench.py), synthetic TPC-H tables at --sf (default 100).

Descriptors, ONE per process (--desc):
  q1              the unchanged Q1-shaped descriptor of plan_bench.py.
  q6              bench.py's Q6 plan: three range preds, two aggregates.
  year_left       revenue per order year through a LEFT join (the
                  descriptor of plan_outer_bench.py).
                  These three have no clause and are the controls against
                  the parent commit: same kernels, same program text.
  q6_in           q6 with the pred ("disc", 5, 8) written as the clause
                  disc IN (5, 6, 7): same rows, same columns, so the
                  difference is the compare code alone.
  q6_cmp          q6 plus the clause orderkey >= suppkey over two int64
                  columns the plan does not otherwise read (true on nearly
                  every row): 16 more bytes per row.  The synthetic lineitem
                  has one date column only, so two key columns stand in for
                  Q12's commit / receipt dates.
  year_left_half  year_left with the ON-clause oyear < 1995 (about half of
                  the rows NULL-extended): the base of the next.
  year_left_half_where
                  the same plus the post-join clause
                  oyear IS NULL OR oyear < 1994.

--warmup executes are excluded, then --reps executes are timed one by one
from the plan_scan_agg stat row (device-side events) and reported as median
[min .. max] in microseconds per tier (baked, generic = GG_PLAN_BAKE=0,
interp = GG_PLAN_RTC=0) with the stat row's hbm_bytes_algorithmic per
execute and the effective TB/s it gives.  One JSON line per measurement.

--pkg-root measures another checkout of the package (the parent commit,
built) with this same script; it knows only the controls.  --dump-dir keeps
the generated program text of both stages of each control (GG_PLAN_RTC_DUMP)
for the driver to compare.

--drive is the session: for --rounds rounds it starts, one process after
the other, the branch and then the parent for each control, then the branch
for each new descriptor, so that branch and parent runs interleave and the
parent-versus-parent spread of the same session is on record.  It then
prints the ratios and whether the controls' program text is byte-identical
between branch and parent (the baked stage's code list sorted first: its
order is the compaction's and differs from run to run).  --only restricts
the session to some descriptors.  The driver itself never opens the GPU.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTROLS = ["q1", "q6", "year_left"]
NEW = ["q6_in", "q6_cmp", "year_left_half", "year_left_half_where"]
DESCS = CONTROLS + NEW
# what each new descriptor is compared against, same session
BASE = {"q6_in": "q6", "q6_cmp": "q6",
        "year_left_half_where": "year_left_half"}

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=int, default=100)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--desc", default="q6_in", choices=DESCS)
ap.add_argument("--tiers", default="baked,generic,interp")
ap.add_argument("--pkg-root", default=HERE)
ap.add_argument("--tag", default="")
ap.add_argument("--dump-dir", default="")
ap.add_argument("--drive", action="store_true")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--only", default="",
                help="--drive: comma list of descriptors to run")
ap.add_argument("--parent-root", default="",
                help="--drive: a built checkout of the parent commit")
args = ap.parse_args()


def dump_path(tag, desc):
    return os.path.join(args.dump_dir, f"rtc_{tag}_{desc}.cu")


def program_text(src):
    """a dumped program with the baked codes in ascending order: the second
    stage lists them in the order the compaction happened to emit the
    groups, which differs between two executes of one library"""
    out = []
    for ln in src.splitlines():
        head, brace, rest = ln.partition("GC[NG] = {")
        if brace:
            codes = sorted(rest[:rest.index("}")].split(", "))
            ln = head + brace + ", ".join(codes) + rest[rest.index("}"):]
        out.append(ln)
    return "\n".join(out)


def drive():
    results = []

    def child(tag, desc, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--desc", desc,
               "--tag", tag, "--sf", str(args.sf), "--warmup",
               str(args.warmup), "--reps", str(args.reps), "--tiers",
               args.tiers, "--pkg-root", root]
        if args.dump_dir:
            cmd += ["--dump-dir", args.dump_dir]
        print(f"== plan_where_bench.py --desc {desc} --tag {tag}", flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=600)
        text = r.stdout.decode()
        sys.stdout.write(text)
        sys.stdout.flush()
        if r.returncode != 0:
            # a failed child ends the session: nothing more is started
            sys.exit(f"{tag} {desc}: rc={r.returncode}")
        results.extend(json.loads(ln) for ln in text.splitlines()
                       if ln.startswith("{"))

    only = [d for d in args.only.split(",") if d] or DESCS
    controls = [d for d in CONTROLS if d in only]
    for rnd in range(1, args.rounds + 1):
        for desc in controls:
            child(f"branch-{rnd}", desc, HERE)
            if args.parent_root:
                child(f"parent-{rnd}", desc, args.parent_root)
        for desc in NEW:
            if desc in only:
                child(f"branch-{rnd}", desc, HERE)

    def med(side, desc, tier):
        return [r["median_us"] for r in results
                if r["tag"].startswith(side) and r["desc"] == desc
                and r["tier"] == tier]

    for tier in args.tiers.split(","):
        summary = {"summary": tier}
        for desc in controls:
            b, p = med("branch", desc, tier), med("parent", desc, tier)
            if b and p:
                summary[f"{desc}_branch_over_parent"] = round(
                    statistics.median(b) / statistics.median(p), 4)
                summary[f"{desc}_parent_spread"] = round(
                    (max(p) - min(p)) / statistics.median(p), 4)
                summary[f"{desc}_branch_spread"] = round(
                    (max(b) - min(b)) / statistics.median(b), 4)
        for desc, base in BASE.items():
            b, p = med("branch", desc, tier), med("branch", base, tier)
            if b and p:
                summary[f"{desc}_over_{base}"] = round(
                    statistics.median(b) / statistics.median(p), 4)
        print(json.dumps(summary), flush=True)
    if args.dump_dir and args.parent_root:
        same = {}
        for desc in controls:
            texts = []
            for tag in ("branch-1", "parent-1"):
                with open(dump_path(tag, desc)) as f:
                    texts.append(hashlib.sha256(
                        program_text(f.read()).encode()).hexdigest())
            same[desc] = {"identical": texts[0] == texts[1],
                          "sha256": texts[0][:16]}
        print(json.dumps({"rtc_text_branch_vs_parent": same}), flush=True)
    print("PLAN_WHERE_BENCH_OK")


if args.drive:
    drive()
    sys.exit(0)

sys.path.insert(0, args.pkg_root)
from greengage_amd import Engine, PGDate, pgdate  # noqa: E402

NEG_INF = -(1 << 63)
REV = ("sum", [("price", "id"), ("disc", "sub100")])
Q1 = ["count", ("sum", [("qty", "id")]), ("sum", [("price", "id")]),
      ("sum", [("disc", "id")]), REV,
      ("sum", [("price", "id"), ("disc", "sub100"), ("tax", "add100")])]
Q6_AGGS = [("sum", [("price", "id"), ("disc", "id")]), "count"]
HALF = [("oyear", NEG_INF, 1995)]

eng = Engine(device=0, n_segments=1, segment_id=0)
li = eng.register_synth("lineitem", seed=42, sf=args.sf)
rows = eng.table_nrows(li)
oy = None
if args.desc.startswith("year"):
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


def compile_desc(name):
    if name == "q1":
        return eng.compile_plan(
            li, preds=[("shipdate", NEG_INF, PGDate("1998-08-15") + 1)],
            group_cols=["rflag", "lstatus"], aggs=Q1)
    if name.startswith("q6"):
        dates = ("shipdate", pgdate(1994, 1, 1), pgdate(1995, 1, 1))
        qty = ("qty", NEG_INF, 2400)
        if name == "q6":
            return eng.compile_plan(li, preds=[dates, ("disc", 5, 8), qty],
                                    aggs=Q6_AGGS)
        if name == "q6_in":
            return eng.compile_plan(li, preds=[dates, qty], aggs=Q6_AGGS,
                                    where=[("in", "disc", [5, 6, 7])])
        return eng.compile_plan(
            li, preds=[dates, ("disc", 5, 8), qty], aggs=Q6_AGGS,
            where=[("cmp", "orderkey", ">=", "suppkey")])
    join = {"table": oy, "build_key": "orderkey", "probe_key": "orderkey",
            "kind": "left",
            "preds": [] if name == "year_left" else list(HALF)}
    kw = {}
    if name == "year_left_half_where":
        kw["where"] = [[("is_null", (0, "oyear")),
                        ("range", (0, "oyear"), NEG_INF, 1994)]]
    return eng.compile_plan(li, joins=[join], group_cols=[(0, "oyear")],
                            aggs=[REV, "count"], **kw)


def stat(p, name):
    for s in eng.stats(p):
        if s["name"] == name:
            return s["total_ms"], s["launches"], s["hbm_bytes_algorithmic"]
    return 0.0, 0, 0


def measure(name, tier):
    if tier == "generic":
        os.environ["GG_PLAN_BAKE"] = "0"
    elif tier == "interp":
        os.environ["GG_PLAN_RTC"] = "0"
    # the control's program text: both stages of a grouped plan, the one
    # stage of an ungrouped one
    if args.dump_dir and name in CONTROLS and tier == (
            "generic" if name.startswith("q6") else "baked"):
        os.environ["GG_PLAN_RTC_DUMP"] = dump_path(args.tag, name)
    try:
        p = compile_desc(name)
        first = eng.execute_plan(p, max_groups=64)
        for _ in range(args.warmup):
            assert eng.execute_plan(p, max_groups=64) == first
        us = []
        for _ in range(args.reps):
            t0, l0, h0 = stat(p, "plan_scan_agg")
            eng.execute_plan(p, max_groups=64)
            t1, l1, h1 = stat(p, "plan_scan_agg")
            assert l1 == l0 + 1
            us.append((t1 - t0) * 1000.0)
    finally:
        for v in ("GG_PLAN_BAKE", "GG_PLAN_RTC", "GG_PLAN_RTC_DUMP"):
            os.environ.pop(v, None)
    m = statistics.median(us)
    print(json.dumps({
        "tag": args.tag, "desc": name, "tier": tier, "sf": args.sf,
        "rows": rows, "warmup": args.warmup, "reps": args.reps,
        "median_us": round(m, 1),
        "min_us": round(min(us), 1), "max_us": round(max(us), 1),
        "hbm_bytes_algorithmic": h1 - h0,
        "effective_tb_s": round((h1 - h0) / (m * 1e-6) / 1e12, 3),
        "paths": sorted(s["name"] for s in eng.stats(p)
                        if s["name"].startswith("path")),
        "groups": len(first),
        # COUNT(*) over all groups: first aggregate of q1, else the second
        "rows_counted": sum(g[2][0 if name == "q1" else 1] for g in first)}),
        flush=True)
    return first


# ungrouped plans are never baked: one generated tier
tiers = [t for t in args.tiers.split(",")
         if not (args.desc.startswith("q6") and t == "baked")]
firsts = [measure(args.desc, t) for t in tiers]
assert all(f == firsts[0] for f in firsts), "tiers disagree"
eng.shutdown()
