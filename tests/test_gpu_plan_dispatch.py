"""Every instantiation of the interpreted plan kernel, through its launcher.

plan.hip launches k_plan_scan_agg<NT, MM, PL, GP, FL> through a table of 48
host launchers indexed by the flags launch_plan_scan_agg derives from the
plan.  One case per table entry: a plan that derives exactly those flags,
run on the interpreted kernel (plan_mode("interp")), two executes, compared
bit for bit with plan_outer_ref.eval_plan.

    NT  GG_PLAN_NT=1 around the executes (nontemporal predicate loads)
    MM  a MIN and a MAX aggregate
    PL  0: no join (NT = 0 cases) or a SEMI join (NT = 1 cases);
        1: a dense INNER join with a payload factor;
        2: a LEFT join with a payload factor plus an ANTI join
    GP  grouped by an (int32, int64) pair, else by a (char1, char1) pair
    FL  one filtered aggregate

A wrong table entry must fail the comparison, so _case checks on the CPU,
before anything is launched, that the expected result differs from what the
neighbouring kernel would give: the filter ignored (FL), the packed pair
coded as e0 * 512 + e1 (GP), the MIN/MAX words added instead of maximised
(MM), the payload column read at the driving row or the LEFT and ANTI joins
taken for INNER and SEMI ones (PL).  NT = 1 and NT = 0 give equal results;
that bit is pinned by the static_asserts beside the table.

Shapes: 3001 driving rows = 12 blocks of 256 threads, the last one partial,
all in the tail loop, whose body is the main loop's; one predicate column of
each width (char1, int32, int64), the three arms of pl_ld<NT>.  The build
table has 3001 rows as well: a kernel that indexed a payload column by the
driving row would read a wrong value inside the column, never past it.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from plan_filter_ref import split
from plan_outer_ref import (NULL_KEY, POS_INF, eval_plan, join, null_extended,
                            register, resolve_joins, run)

pytestmark = pytest.mark.gpu

N = M = 3001
MSB = 1 << 63
U64 = (1 << 64) - 1
PREDS = [("pc", 1, 10), ("pi", -90, 101), ("pl", 50, POS_INF)]
FILTER = [("f", 3, 7)]
COMBOS = [(nt, mm, pl, gp, fl) for fl in (0, 1) for gp in (0, 1)
          for nt in (0, 1) for mm in (0, 1) for pl in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def _tables():
    """{table: (columns as register() takes them, null map)}"""
    rng = np.random.default_rng(4800)
    bk = (rng.permutation(np.arange(2 * M))[:M] + 1).astype(np.int64)
    drive = [("pc", "char1", rng.integers(0, 10, N).astype(np.uint8)),
             ("pi", "int32", rng.integers(-100, 101, N).astype(np.int32)),
             ("pl", "int64", rng.integers(0, 1000, N).astype(np.int64)),
             ("fk", "int64", rng.integers(-3, 2 * M + 6, N).astype(np.int64)),
             ("fk2", "int64", rng.integers(0, 100, N).astype(np.int64)),
             ("g", "char1", rng.integers(0, 4, N).astype(np.uint8)),
             ("h", "char1", rng.integers(0, 3, N).astype(np.uint8)),
             ("a", "int32", rng.integers(-3, 4, N).astype(np.int32)),
             ("b", "int64", ((1 << 40) + rng.integers(0, 3, N))
              .astype(np.int64)),
             ("x", "int64", rng.integers(0, 1000, N).astype(np.int64)),
             ("y", "int32", rng.integers(-500, 500, N).astype(np.int32)),
             ("f", "int32", rng.integers(0, 10, N).astype(np.int32))]
    build = [("bk", "int64", bk),
             ("ak", "int64", rng.integers(0, 50, M).astype(np.int64)),
             ("w", "int64", rng.integers(1, 1000, M).astype(np.int64))]
    return {"pd_drive": (drive, {"y": rng.random(N) < 0.1,
                                 "b": rng.random(N) < 0.05}),
            "pd_build": (build, {})}


def _host(name):
    """(data, nulls) of a table in the evaluator's form"""
    cols, nullmap = _tables()[name]
    data = {c: np.asarray(a).astype(np.int64) for c, _ty, a in cols}
    nulls = {c: np.asarray(nullmap.get(c, np.zeros(len(a), bool))).astype(bool)
             for c, _ty, a in cols}
    return data, nulls


def _plan(nt, mm, pl, gp, fl, bt=None):
    """(joins, group columns, aggregates) of one combination"""
    bd, bn = _host("pd_build")
    if pl == 2:
        joins = [join(bt, bd, bn, "bk", "fk", kind="left"),
                 join(bt, bd, bn, "ak", "fk2", kind="anti")]
    elif pl == 1:
        joins = [join(bt, bd, bn, "bk", "fk", kind="inner")]
    else:
        joins = [join(bt, bd, bn, "ak", "fk2", kind="semi")] if nt else []
    aggs = ["count", ("sum", [("x", "id"), ((0, "w"), "id") if pl
                              else ("y", "add100")])]
    if mm:
        aggs += [("min", ("y", "id")), ("max", ("x", "sub100"))]
    if fl:
        aggs.append(("filter", ("sum", [("x", "id")]), FILTER))
    return joins, ["a", "b"] if gp else ["g", "h"], aggs


def _decode(word, kind):
    e = (word ^ U64) if kind == "min" else word
    return (e ^ MSB) - (1 << 64 if (e ^ MSB) >= MSB else 0)


@functools.lru_cache(maxsize=None)
def _case(nt, mm, pl, gp, fl):
    """the expected result, after checking that it tells this combination's
    kernel from its neighbours'"""
    data, nulls = _host("pd_drive")
    joins, group_cols, aggs = _plan(nt, mm, pl, gp, fl)
    exp = eval_plan(N, data, nulls, PREDS, joins, group_cols, aggs)
    live, ridx = resolve_joins(N, data, nulls, PREDS, joins)
    rows = np.nonzero(live)[0]
    assert len(exp) > 1 and 0 < len(rows) < N
    if fl:
        plain = [split(a)[0] for a in aggs]
        assert eval_plan(N, data, nulls, PREDS, joins, group_cols,
                         plain) != exp
    if gp:
        # e0 * 512 + e1 over the values (NULL = 256), decoded as the packed
        # code (e0 << shift) | e1 with e = value - column minimum + 1
        e = [np.where(nulls[c][rows], 256, data[c][rows]) for c in group_cols]
        gmin = [int(data[c].min()) for c in group_cols]
        shift = (int(data["b"].max()) - gmin[1] + 1).bit_length()
        wrong = set()
        for code in (e[0] * 512 + e[1]).tolist():
            e0, e1 = (code & U64) >> shift, code & ((1 << shift) - 1)
            wrong.add((gmin[0] + e0 - 1 if e0 else NULL_KEY,
                       gmin[1] + e1 - 1 if e1 else NULL_KEY))
        assert wrong != {(k0, k1) for k0, k1, _vals in exp}
    if mm:
        # each group's order-encoded words (MAX: x ^ msb, MIN: its
        # complement) added modulo 2^64; they follow "count" and the SUM
        keys = [np.where(nulls[c][rows], NULL_KEY, data[c][rows])
                for c in group_cols]
        differs = 0
        for k0, k1, vals in exp:
            sel = rows[(keys[0] == k0) & (keys[1] == k1)]
            for slot, kind, col, val in [(2, "min", "y", data["y"]),
                                         (3, "max", "x", 100 - data["x"])]:
                words = [(int(v) & U64) ^ MSB ^ (U64 if kind == "min" else 0)
                         for v in val[sel[~nulls[col][sel]]]]
                if words:
                    assert _decode(max(words), kind) == vals[slot]
                    differs += _decode(sum(words) & U64, kind) != vals[slot]
        assert differs
    if pl:
        # the payload factor at the driving row is another value
        hit = rows[ridx[0][rows] >= 0]
        w = _host("pd_build")[0]["w"]
        assert np.any(w[hit] != w[ridx[0][hit]])
    if pl == 2:
        # LEFT is not INNER: some rows are NULL-extended; ANTI drops rows
        kept, extended = null_extended(N, data, nulls, PREDS, joins)[0]
        assert 0 < extended < kept
        assert kept < np.count_nonzero(
            resolve_joins(N, data, nulls, PREDS, joins[:1])[0])
    elif joins:
        # INNER and SEMI drop rows
        assert len(rows) < np.count_nonzero(
            resolve_joins(N, data, nulls, PREDS, [])[0])
    return exp


@contextlib.contextmanager
def plan_nt(on):
    """GG_PLAN_NT=1 selects the NT = 1 kernels; read at every launch"""
    old = os.environ.pop("GG_PLAN_NT", None)
    if on:
        os.environ["GG_PLAN_NT"] = "1"
    try:
        yield
    finally:
        os.environ.pop("GG_PLAN_NT", None)
        if old is not None:
            os.environ["GG_PLAN_NT"] = old


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


@pytest.fixture(scope="module")
def tables(eng):
    return {name: register(eng, name, cols, nullmap)[0]
            for name, (cols, nullmap) in _tables().items()}


@pytest.mark.parametrize("nt,mm,pl,gp,fl", COMBOS)
def test_dispatch(eng, tables, nt, mm, pl, gp, fl):
    exp = _case(nt, mm, pl, gp, fl)
    data, nulls = _host("pd_drive")
    joins, group_cols, aggs = _plan(nt, mm, pl, gp, fl, tables["pd_build"])
    with plan_nt(nt):
        _p, _exp, paths = run(eng, "interp", tables["pd_drive"], data, nulls,
                              PREDS, joins, group_cols, aggs, repeats=2,
                              exp=exp)
    assert "path_plan_interp" in paths
