"""Two-word carries on every accumulator destination of compiled plans.

The add-with-carry helper (plan.hip pl_atomic_add128 / pl_add128 and
their twins in the generated program's prelude) is the single point of
failure of every exact sum.  These cases force the low word to carry,
in both directions, on each destination it serves: register
accumulators and the wave flush (no group column), the generic LDS
cache and the baked 2-word table (2x2 char1 groups), and the global
table transition (more groups than the LDS cache holds).

Two int64 columns in +-3e9, ~10% NULLs in `a`; single products reach
+-9e18, so a handful of rows cross 2^64 and the signed running sum
wanders through zero.  test_cases_force_carries pins that on the CPU:
in every case some group's |SUM(a*b)| exceeds 2^64 and some group's
running sum changes sign (n = 1 cannot: one product is below 2^63; it
is there for the single-lane wave flush).  Reference: exact big-int
evaluation in plan_minmax_ref; all comparisons are bit-exact, on the
hipRTC path and on the interpreted kernel.
"""
import numpy as np
import pytest

from plan_minmax_ref import eval_plan, register, run

AGGS = [("sum", [("a", "id"), ("b", "id")]), ("sum", [("a", "id")]),
        "count", ("count", "a")]
TINY = [1, 63, 64, 65, 300]


def _ab(rng, n):
    """a, b in +-3e9 with signs agreeing on ~3 rows of 4, so sums drift
    past 2^64 quickly while single rows still pull them back"""
    a = rng.integers(-3 * 10 ** 9, 3 * 10 ** 9, n).astype(np.int64)
    b = rng.integers(1, 3 * 10 ** 9, n).astype(np.int64)
    b = np.where(rng.random(n) < 0.75, np.sign(a) * b, -np.sign(a) * b)
    return a, b.astype(np.int64), rng.random(n) < 0.1


def _tiny(n):
    # seeds fixed so that test_cases_force_carries holds for every n
    a, b, an = _ab(np.random.default_rng(133 + n), n)
    if n == 1:
        an[:] = False
    return [("a", "int64", a), ("b", "int64", b)], {"a": an}, []


def _char_groups():
    rng = np.random.default_rng(21)
    n = 5000
    a, b, an = _ab(rng, n)
    g0 = rng.choice(np.frombuffer(b"AN", np.uint8), n)
    g1 = rng.choice(np.frombuffer(b"FO", np.uint8), n)
    return ([("g0", "char1", g0), ("g1", "char1", g1), ("a", "int64", a),
             ("b", "int64", b)], {"a": an}, ["g0", "g1"])


def _many_groups():
    rng = np.random.default_rng(22)
    n = 20000
    a, b, an = _ab(rng, n)
    k = (rng.integers(0, 500, n) * 7919 - 100000).astype(np.int64)
    return ([("k", "int64", k), ("a", "int64", a), ("b", "int64", b)],
            {"a": an}, ["k"])


_CASES = {}


def _case(name):
    """(cols, nullmap, group_cols, expected), built once per case and
    shared by both modes"""
    if name not in _CASES:
        cols, nullmap, gcols = (_char_groups() if name == "char"
                                else _many_groups() if name == "many"
                                else _tiny(name))
        n = len(cols[0][2])
        data = {c: np.asarray(v).astype(np.int64) for c, _t, v in cols}
        nulls = {c: np.asarray(nullmap.get(c, np.zeros(n, bool)), bool)
                 for c in data}
        _CASES[name] = (cols, nullmap, gcols,
                        eval_plan(n, data, nulls, [], [], gcols, AGGS))
    return _CASES[name]


def test_cases_force_carries():
    for name in TINY[1:] + ["char", "many"]:
        cols, nullmap, gcols, exp = _case(name)
        assert max(abs(g[2][0]) for g in exp) > 1 << 64, name
        data = {c: np.asarray(v).astype(np.int64) for c, _t, v in cols}
        keys = (np.zeros(len(data["a"]), np.int64) if not gcols else
                sum(data[c] * 1000 ** i for i, c in enumerate(gcols)))
        flips = 0
        for k in np.unique(keys):
            rows = np.nonzero((keys == k) & ~nullmap["a"])[0]
            run_sum, signs = 0, set()
            for x, y in zip(data["a"][rows].tolist(),
                            data["b"][rows].tolist()):
                run_sum += x * y
                signs.add(run_sum > 0)
            flips += len(signs) == 2
        assert flips, name


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from greengage_amd import Engine
    e = Engine()
    yield e
    e.shutdown()


@pytest.fixture(params=["rtc", "interp"])
def mode(request):
    return request.param


def _run(eng, mode, name, repeats=1):
    cols, nullmap, gcols, exp = _case(name)
    t, data, nulls = register(eng, f"carry_{name}_{mode}", cols, nullmap)
    p, _exp = run(eng, mode, t, data, nulls, [], gcols, AGGS,
                  repeats=repeats, exp=exp)
    return {s["name"] for s in eng.stats(p)}, exp


@pytest.mark.gpu
@pytest.mark.parametrize("n", TINY)
def test_register_add_and_wave_flush(eng, mode, n):
    _run(eng, mode, n)


@pytest.mark.gpu
def test_lds_cache_then_baked_two_word(eng, mode):
    """SUM over negative values defeats the fast-tier proof: the first
    execute runs the generic LDS cache, the repeats the baked 2-word
    table."""
    paths, exp = _run(eng, mode, "char", repeats=4)
    assert len(exp) == 4
    assert paths & {"path_plan_rtc_baked", "path_plan_interp"}
    assert "path_plan_rtc_baked_fast" not in paths
    if mode == "rtc":
        assert "path_plan_rtc_baked" in paths


@pytest.mark.gpu
def test_global_table_transition(eng, mode):
    """~500 groups overflow the 32-slot block cache, so most rows add
    straight into the global table."""
    _paths, exp = _run(eng, mode, "many")
    assert len(exp) > 400
