"""HAVING of compiled plans (engine_abi.h gg_plan_having), without a GPU:
the extension's layout in the binding's mirror, the builder's sugar, limits
and errors, the reference (plan_having_ref) by hand, and THE row test of
greengage_amd/csrc/plan_having.h, which the device kernel and the host path
share, compiled into a stand-alone program (plan_having_host_main.cpp, its
own main, built with the address and undefined-behaviour sanitizers where
the compiler has their runtimes) and driven over stdin against the
reference.
"""
import ctypes
import itertools
import os
import random
import re
import shutil
import subprocess

import pytest

from plan_having_ref import (I128_MAX, I128_MIN, atom_true, filter_groups,
                             passes)

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
M64 = (1 << 64) - 1
MSB = 1 << 63
KIND = {"range": 0, "not_range": 1, "is_null": 2, "not_null": 3}
I128, VMIN, VMAX = 0, 1, 2          # gg::PlanHavingVal


def _header():
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        return f.read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, _header()).group(1))


def _atoms(h):
    """the used part of a _PlanHaving: [[(kind, agg, lo, hi)]] with the
    bounds as Python ints"""
    def i128(lo, hi):
        return (hi << 64) | lo
    return [[(a.kind, a.agg, i128(a.lo_lo, a.lo_hi), i128(a.hi_lo, a.hi_hi))
             for a in list(h.clauses[c].atoms)[:h.clauses[c].natoms]]
            for c in range(h.nclauses)]


# ---- layout and constants ----

def test_having_layout_matches_library():
    from greengage_amd import engine as ge
    assert (ctypes.sizeof(ge._PlanHaving)
            == ge.lib().gg_engine_plan_having_size())
    assert [f for f, _t in ge._PlanHavingAtom._fields_] == [
        "lo_lo", "lo_hi", "hi_lo", "hi_hi", "kind", "agg"]
    assert [f for f, _t in ge._PlanHavingClause._fields_] == [
        "atoms", "natoms"]
    assert [f for f, _t in ge._PlanHaving._fields_] == ["clauses", "nclauses"]
    assert ctypes.sizeof(ge._PlanHavingAtom) == 40
    assert ge._PlanHavingClause.natoms.offset == 40 * ge.PLAN_MAX_HAVING_ATOMS
    # the descriptor and the WHERE keep their layouts
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()
    assert [f for f, _t in ge._PlanDesc._fields_][-1] == "est_groups"
    assert ctypes.sizeof(ge._PlanWhere) == ge.lib().gg_engine_plan_where_size()


def test_constants_match_header():
    import greengage_amd as g
    from greengage_amd import engine as ge
    assert ge.PLAN_MAX_HAVING_CLAUSES == _define(
        "GG_PLAN_MAX_HAVING_CLAUSES") == 4
    assert ge.PLAN_MAX_HAVING_ATOMS == _define("GG_PLAN_MAX_HAVING_ATOMS") == 4
    assert ge.PLAN_MAX_HAVING_TOTAL == _define("GG_PLAN_MAX_HAVING_TOTAL") == 8
    assert g.PLAN_MAX_HAVING_CLAUSES == 4 and g.PLAN_MAX_HAVING_TOTAL == 8
    assert g.PLAN_MAX_HAVING_ATOMS == 4
    src = _header()
    for name in ("RANGE", "NOT_RANGE", "IS_NULL", "NOT_NULL"):
        v = int(re.search(r"GG_HAVING_%s\s*=\s*(\d+)" % name, src).group(1))
        assert getattr(ge, "HAVING_" + name) == v == KIND[name.lower()]
        assert getattr(g, "HAVING_" + name) == v
    assert g.HAVING_NEG_INF == I128_MIN and g.HAVING_POS_INF == I128_MAX
    assert g.build_plan_having is ge.build_plan_having


# ---- the builder ----

AGGS = ["count", ("sum", [("x", "id")]), ("min", ("m", "id")),
        ("avg", [("x", "id")]),
        ("filter", ("max", ("m", "id")), [("x", 0, 5)]),
        ("filter", ("avg", [("x", "id")]), [("x", 0, 5)])]


def test_builder_sugar_and_sentinels():
    from greengage_amd import engine as ge
    R, NR = ge.HAVING_RANGE, ge.HAVING_NOT_RANGE
    big = (1 << 64) + 1
    h = ge.build_plan_having(AGGS, [
        ("range", 0, 1, 5),
        [("not_range", 1, -big, big), ("is_null", 2), ("not_null", 4)],
        [("in", 1, [-6, big]), ("cmp", 0, "=", 0)],
        ("range", 1, I128_MIN, I128_MAX)])
    assert _atoms(h) == [
        [(R, 0, 1, 5)],
        [(NR, 1, -big, big), (ge.HAVING_IS_NULL, 2, 0, 0),
         (ge.HAVING_NOT_NULL, 4, 0, 0)],
        [(R, 1, -6, -5), (R, 1, big, big + 1), (R, 0, 0, 1)],
        [(R, 1, I128_MIN, I128_MAX)]]
    # the two halves as the ABI stores them
    a = h.clauses[1].atoms[0]
    assert (a.lo_lo, a.lo_hi, a.hi_lo, a.hi_hi) == (M64, -2, 1, 1)


@pytest.mark.parametrize("v", [0, -1, 300, -(1 << 64) - 1, (1 << 100)])
def test_builder_compare_ops(v):
    from greengage_amd import engine as ge
    R, NR = ge.HAVING_RANGE, ge.HAVING_NOT_RANGE
    got = {op: _atoms(ge.build_plan_having(AGGS, [("cmp", 1, op, v)]))
           for op in ("<", "<=", "=", "<>", ">", ">=")}
    assert got == {"<": [[(R, 1, I128_MIN, v)]],
                   "<=": [[(R, 1, I128_MIN, v + 1)]],
                   "=": [[(R, 1, v, v + 1)]],
                   "<>": [[(NR, 1, v, v + 1)]],
                   ">": [[(R, 1, v + 1, I128_MAX)]],
                   ">=": [[(R, 1, v, I128_MAX)]]}


def test_builder_errors():
    from greengage_amd import engine as ge
    one = ("cmp", 0, ">", 1)
    assert ge.build_plan_having(AGGS, [one] * 4).nclauses == 4
    with pytest.raises(ValueError):
        ge.build_plan_having(AGGS, [one] * 5)
    assert ge.build_plan_having(AGGS, [[one] * 4]).clauses[0].natoms == 4
    with pytest.raises(ValueError):
        ge.build_plan_having(AGGS, [[one] * 5])
    with pytest.raises(ValueError):        # an IN-list counts per value
        ge.build_plan_having(AGGS, [("in", 0, [1, 2, 3, 4, 5])])
    assert ge.build_plan_having(AGGS, [[one] * 4, [one] * 4]).nclauses == 2
    with pytest.raises(ValueError):        # 9 atoms in all
        ge.build_plan_having(AGGS, [[one] * 4, [one] * 4, one])
    with pytest.raises(ValueError):        # an empty disjunction
        ge.build_plan_having(AGGS, [[]])
    with pytest.raises(ValueError):        # unknown atoms
        ge.build_plan_having(AGGS, [("eq", 0, 1)])
    with pytest.raises(ValueError):
        ge.build_plan_having(AGGS, [("cmp", 0, "!=", 1)])
    for a in (3, 5):                       # an AVG, plain and FILTERed
        with pytest.raises(ValueError):
            ge.build_plan_having(AGGS, [("not_null", a)])
    for a in (-1, 6):
        with pytest.raises(ValueError):
            ge.build_plan_having(AGGS, [("not_null", a)])
    # v + 1 would leave 128 bits
    for atom in (("cmp", 0, "<=", I128_MAX), ("cmp", 0, "=", I128_MAX),
                 ("cmp", 0, "<>", I128_MAX), ("cmp", 0, ">", I128_MAX),
                 ("in", 0, [1, I128_MAX])):
        with pytest.raises(ValueError):
            ge.build_plan_having(AGGS, [atom])
    assert _atoms(ge.build_plan_having(AGGS, [("cmp", 0, ">=", I128_MAX)])) \
        == [[(ge.HAVING_RANGE, 0, I128_MAX, I128_MAX)]]
    for lo, hi in ((I128_MIN - 1, 0), (0, I128_MAX + 1)):
        with pytest.raises(ValueError):
            ge.build_plan_having(AGGS, [("range", 0, lo, hi)])


def test_no_clause_is_no_extension():
    from greengage_amd import engine as ge
    assert ge.build_plan_having().nclauses == 0
    assert ge.build_plan_having(AGGS, ()).nclauses == 0
    assert bytes(ge.build_plan_having(AGGS, [])) == bytes(ge._PlanHaving())


# ---- the reference by hand ----

def test_reference_by_hand():
    groups = [(1, 0, [3, -5, None]), (2, 0, [1, 1 << 70, 7]),
              (3, 0, [2, 0, -7])]

    def keys(having):
        return [g[0] for g in filter_groups(groups, having)]
    assert keys([]) == [1, 2, 3]
    assert keys([("cmp", 0, ">=", 2)]) == [1, 3]
    assert keys([("cmp", 1, ">", 1 << 64)]) == [2]
    assert keys([("range", 2, -7, 7)]) == [3]
    assert keys([("not_range", 2, -7, 7)]) == [2]     # NULL: not true
    assert keys([("is_null", 2)]) == [1]
    assert keys([("not_null", 2)]) == [2, 3]
    assert keys([("is_null", 0)]) == []
    assert keys([[("is_null", 2), ("cmp", 2, "<", 0)]]) == [1, 3]
    assert keys([("in", 0, [1, 3]), ("cmp", 1, "<>", -5)]) == [2]
    assert keys([("range", 1, 5, 5)]) == []           # lo == hi: empty
    assert keys([("not_range", 1, 5, -5)]) == [1, 2, 3]
    assert keys([("range", 1, I128_MIN, I128_MAX)]) == [1, 2, 3]
    with pytest.raises(AssertionError):
        passes([("not_null", 0)], [(5, 1)])           # an AVG tuple


# ---- the shared row test, stand-alone ----

@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("having") / "plan_having_host")
    src = os.path.join(HERE, "plan_having_host_main.cpp")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        # a compiler without the sanitizer runtimes: the plain program
        subprocess.run(base, check=True)

    def ask(lines):
        r = subprocess.run([out], input="".join(s + "\n" for s in lines),
                           capture_output=True, text=True, check=True)
        assert r.stderr == ""
        ans = r.stdout.split("\n")[:-1]
        assert len(ans) == len(lines)
        return ans
    return ask


def _halves(v):
    """a signed 128-bit value as 'hi lo' (signed, unsigned)"""
    return f"{v >> 64} {v & M64}"


def _atom_text(tag, val, slot, cnt, lo, hi):
    return f"{KIND[tag]} {val} {slot} {cnt} {_halves(lo)} {_halves(hi)}"


def _word(val, x):
    """the accumulator word of a MIN / MAX whose value is the int64 x"""
    w = (x & M64) ^ MSB
    return w ^ M64 if val == VMIN else w


EDGES = [0, 1, -1, 1 << 63, -(1 << 63), 1 << 64, -(1 << 64), (1 << 64) + 1,
         -((1 << 64) + 1), I128_MIN, I128_MAX]
TAGS = ["range", "not_range", "is_null", "not_null"]


def _bound_pairs(tag):
    if tag in ("is_null", "not_null"):
        return [(0, 0)]
    return list(itertools.product(EDGES, EDGES))


def test_row_test_i128_edges(prog):
    """COUNT / SUM values: every kind over every value and bound pair of
    EDGES, which holds both sentinels, lo == hi and lo > hi"""
    lines, exp, empty, full = [], [], 0, 0
    for tag in TAGS:
        for lo, hi in _bound_pairs(tag):
            for v in EDGES:
                lines.append(f"R 1 1 {_atom_text(tag, I128, 0, 0, lo, hi)} "
                             f"3 77 {v & M64} {(v >> 64) & M64}")
                e = atom_true((tag, 0, lo, hi), [v])
                exp.append(str(int(e)))
                if lo > hi and tag == "range":
                    assert not e
                    empty += 1
                if lo >= hi and hi != I128_MAX and tag == "not_range":
                    assert e
                    full += 1
    assert empty > 100 and full > 100
    assert prog(lines) == exp
    assert "0" in exp and "1" in exp


def test_row_test_minmax_edges(prog):
    """MIN / MAX words of INT64_MIN, -1, 0 and INT64_MAX, each with N = 0
    (NULL) and N > 0, every kind, every bound pair"""
    lines, exp = [], []
    for val, tag in itertools.product((VMIN, VMAX), TAGS):
        for lo, hi in _bound_pairs(tag):
            for x, n in itertools.product((INT64_MIN, -1, 0, INT64_MAX),
                                          (0, 3)):
                # slot 1 holds the word, slot 0 the non-NULL count
                lines.append(f"R 1 1 {_atom_text(tag, val, 1, 0, lo, hi)} "
                             f"5 77 {n} 0 {_word(val, x)} 0")
                exp.append(str(int(atom_true((tag, 0, lo, hi),
                                             [x if n else None]))))
    got = prog(lines)
    assert got == exp
    assert "0" in exp and "1" in exp


def test_row_test_cnf_random(prog):
    """random quals within the limits over rows of (COUNT, SUM, MIN, MAX):
    clauses AND, atoms OR, against the reference"""
    rng = random.Random(4711)
    small = [-3, -1, 0, 1, 2, 5, I128_MIN, I128_MAX, 1 << 64, -(1 << 64)]
    lines, exp = [], []
    for _ in range(600):
        vals = [rng.choice([0, 1, 2, 5]), rng.choice(small[:6] + small[8:]),
                rng.choice([None, -3, 0, 2]), rng.choice([None, -1, 1, 5])]
        # accumulators: 0 COUNT, 1 SUM, 2 MIN word, 3 N(min), 4 MAX word,
        # 5 N(max)
        row = [99, vals[0], 0, vals[1] & M64, (vals[1] >> 64) & M64,
               _word(VMIN, vals[2] or 0), 0, int(vals[2] is not None), 0,
               _word(VMAX, vals[3] or 0), 0, int(vals[3] is not None), 0]
        where = {0: (I128, 0, 0), 1: (I128, 1, 0), 2: (VMIN, 2, 3),
                 3: (VMAX, 4, 5)}
        nat = [rng.randint(1, 4) for _ in range(rng.randint(1, 4))]
        while sum(nat) > 8:
            nat.pop()
        having, text = [], []
        for n in nat:
            clause = []
            for _q in range(n):
                tag, a = rng.choice(TAGS), rng.randrange(4)
                lo, hi = rng.choice(small), rng.choice(small)
                clause.append((tag, a, lo, hi))
                text.append(_atom_text(tag, *where[a], lo, hi))
            having.append(clause)
        lines.append(f"R {len(nat)} {' '.join(map(str, nat))} "
                     f"{' '.join(text)} {len(row)} "
                     f"{' '.join(map(str, row))}")
        exp.append(str(int(passes(having, vals))))
    assert prog(lines) == exp
    assert exp.count("1") > 50 and exp.count("0") > 50


def test_row_test_driver_rejects_bad_queries(prog):
    assert prog(["X", "R 5 1", "R 1 1 0 0 3 0 0 0 0 0 3 1 2 3"]) == [
        "E", "E", "E"]
