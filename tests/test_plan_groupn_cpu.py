"""Three and four group columns in compiled plans (engine_abi.h
gg_plan_groups), everything that needs no GPU: the binding's layout, the
host's width arithmetic, the builder, the reference evaluator, and the one
decoder (plan_keys.h), which a stand-alone program (plan_groupn_host_main.cpp,
its own main) round-trips against codes packed by hand.  The program is built
twice, plain and with the address and undefined-behaviour sanitizers, and both
builds are executed directly.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import plan_groupn_ref as ref
from plan_groupn_ref import NULL_KEY

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OK, EINVAL, ENOTSUP = 0, 1, 5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- layout ----

def test_groups_binding_matches_the_library():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanGroups) == ge.lib().gg_engine_plan_groups_size()
    with open(os.path.join(REPO, "include", "engine_abi.h")) as f:
        m = re.search(r"#define GG_PLAN_MAX_GROUP_COLS (\d+)", f.read())
    assert int(m.group(1)) == ge.PLAN_MAX_GROUP_COLS == 4


def test_descriptor_keeps_its_layout():
    from greengage_amd import engine as ge
    assert ctypes.sizeof(ge._PlanDesc) == ge.lib().gg_engine_plan_desc_size()
    assert [f for f, _t in ge._PlanDesc._fields_][-1] == "est_groups"
    assert ge._PlanDesc.group_cols.size == 2 * ctypes.sizeof(ctypes.c_char_p)


# ---- gg_engine_plan_group_bits_n ----

def _span(bits):
    """(mn, mx) of a column whose width is exactly `bits`"""
    return 0, (1 << bits) - 2 if bits > 1 else 0


def test_bits_n_agrees_with_the_pair_function():
    from greengage_amd import plan_group_bits, plan_group_bits_n
    rng = np.random.default_rng(7)
    cases = [((0, 0), (0, 0)), ((5, 5), (4, 4)), ((-7, 1 << 33), (8, 1 << 40)),
             ((0, 0), ((1 << 31) - 2, (1 << 31) - 2)),
             ((0, 0), ((1 << 31) - 2, (1 << 31) - 1)),
             ((I64_MIN, 0), (I64_MAX, 0)), ((I64_MIN, I64_MIN), (I64_MAX, I64_MAX))]
    for _ in range(40):
        a = sorted(int(x) for x in rng.integers(-(1 << 62), 1 << 62, 2))
        b = sorted(int(x) for x in rng.integers(-(1 << 20), 1 << 20, 2))
        cases.append(((a[0], b[0]), (a[1], b[1])))
    for mn, mx in cases:
        assert plan_group_bits_n(mn, mx) == plan_group_bits(mn, mx), (mn, mx)


def test_bits_n_empty_column_and_counts():
    from greengage_amd import plan_group_bits_n
    # mn > mx stands for a column with no rows: one bit, the NULL code alone
    assert plan_group_bits_n((0, 1, 0), (9, 0, 0)) == (OK, (4, 1, 1))
    assert plan_group_bits_n((5,), (5,)) == (OK, (1,))
    assert plan_group_bits_n((0,), ((1 << 62) - 2,)) == (OK, (62,))
    assert plan_group_bits_n((0,), ((1 << 62) - 1,)) == (ENOTSUP, (63,))
    assert plan_group_bits_n((), ())[0] == EINVAL
    assert plan_group_bits_n((0,) * 5, (0,) * 5)[0] == EINVAL


@pytest.mark.parametrize("widths", [(20, 21, 21), (1, 1, 60), (60, 1, 1),
                                    (15, 15, 16, 16), (1, 1, 1, 59),
                                    (31, 29, 1, 1)])
def test_bits_n_budget_edge(widths):
    """widths summing to exactly 62 are accepted; one more bit in any one
    column is refused"""
    from greengage_amd import plan_group_bits_n
    assert sum(widths) == 62
    mn = [_span(b)[0] for b in widths]
    mx = [_span(b)[1] for b in widths]
    assert plan_group_bits_n(mn, mx) == (OK, widths)
    for g in range(len(widths)):
        mx2 = list(mx)
        mx2[g] = _span(widths[g] + 1)[1]
        over = tuple(b + (i == g) for i, b in enumerate(widths))
        assert plan_group_bits_n(mn, mx2) == (ENOTSUP, over)


def test_bits_n_full_range_columns_do_not_overflow():
    from greengage_amd import plan_group_bits_n
    for n in (3, 4):
        assert plan_group_bits_n((I64_MIN,) * n, (I64_MAX,) * n) == \
            (ENOTSUP, (65,) * n)
    assert plan_group_bits_n((I64_MIN, 0, -1), (I64_MAX - 1, 0, I64_MAX)) == \
        (ENOTSUP, (64, 1, 64))
    assert plan_group_bits_n((I64_MIN + 2, 3, 3, 3),
                             (I64_MIN + 2 + (1 << 58), 3, 3, 3)) == \
        (OK, (59, 1, 1, 1))


# ---- the builders ----

def _desc_bytes(d):
    return bytes((ctypes.c_char * ctypes.sizeof(d)).from_buffer_copy(d))


def test_descriptor_bytes_for_up_to_two_columns():
    """build_plan_desc fills what it always filled: for <= 2 columns the
    descriptor is the one the two-column code path builds by hand, and a
    third column changes none of its bytes"""
    from greengage_amd import engine as ge
    kw = dict(preds=[("d", 0, 10)], aggs=["count", ("sum", [("v", "id")])],
              joins=[{"table": 1, "build_key": "k", "probe_key": "fk",
                      "kind": "inner"}])
    for cols in ([], ["a"], ["a", (0, "b")]):
        d, kinds = ge.build_plan_desc(0, group_cols=cols, **kw)
        hand, _k = ge.build_plan_desc(0, group_cols=[], **kw)
        hand.ngroup = len(cols)
        for g, c in enumerate(cols):
            hand.group_cols[g] = (c if isinstance(c, str) else c[1]).encode()
            hand.group_src[g] = 0 if isinstance(c, str) else 1 + c[0]
        assert d.ngroup == len(cols) and kinds == [ge.AGG_COUNT_STAR, ge.AGG_SUM]
        assert [d.group_cols[g] for g in range(2)] == \
            [hand.group_cols[g] for g in range(2)]
        assert list(d.group_src) == list(hand.group_src)
        assert ge.build_plan_groups(cols).ncols == 0
    two, _k = ge.build_plan_desc(0, group_cols=["a", (0, "b")], **kw)
    three, _k = ge.build_plan_desc(0, group_cols=["a", (0, "b"), "c"], **kw)
    assert three.ngroup == 2
    # pointers aside, the bytes are the same: compare every scalar field
    for f, _t in ge._PlanDesc._fields_:
        if f in ("scan", "joins", "aggs", "filters", "order", "group_cols"):
            continue
        a, b = getattr(two, f), getattr(three, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else a == b, f
    assert list(three.group_cols) == [b"a", b"b"]


def test_build_plan_groups():
    from greengage_amd import engine as ge
    g = ge.build_plan_groups(["a", "b", (1, "c")])
    assert (g.ncols, g.cols[0], g.src[0]) == (1, b"c", 2)
    g = ge.build_plan_groups([(0, "x"), "b", "c", (0, "d")])
    assert g.ncols == 2
    assert [(g.cols[i], g.src[i]) for i in range(2)] == [(b"c", 0), (b"d", 1)]
    with pytest.raises(ValueError):
        ge.build_plan_groups(["a", "b", "c", "d", "e"])


# ---- the evaluator ----

def test_reference_by_hand():
    a = np.array([1, 1, 1, 2, 2, 1, 1], np.int64)
    b = np.array([5, 5, 5, 5, 5, 6, 5], np.int64)
    c = np.array([9, 9, 8, 9, 9, 9, 9], np.int64)
    v = np.array([1, 2, 4, 8, 16, 32, 64], np.int64)
    data = {"a": a, "b": b, "c": c, "v": v}
    nulls = {k: np.zeros(7, bool) for k in data}
    nulls["b"][6] = True          # (1, NULL, 9)
    nulls["c"][4] = True          # (2, 5, NULL)
    got = ref.eval_plan(7, data, nulls, [], [], ["a", "b", "c"],
                        ["count", ("sum", [("v", "id")])])
    assert got == [((1, NULL_KEY, 9), [1, 64]), ((1, 5, 8), [1, 4]),
                   ((1, 5, 9), [2, 3]), ((1, 6, 9), [1, 32]),
                   ((2, 5, NULL_KEY), [1, 16]), ((2, 5, 9), [1, 8])]
    top = ref.order_groups(got, [("key", 2, "desc", "nulls_first"),
                                 ("agg", 1, "desc")], 3)
    # NULL first, then c = 9 (sums 64, 32, 8, 3) ahead of c = 8
    assert [g[0] for g in top] == [(2, 5, NULL_KEY), (1, NULL_KEY, 9),
                                   (1, 6, 9)]
    assert [g[0] for g in ref.filter_groups(got, [("cmp", 1, ">=", 16)])] == \
        [(1, NULL_KEY, 9), (1, 6, 9), (2, 5, NULL_KEY)]
    # the code model: monotone in the tuple, NULL first
    arrays = [a, b, c]
    bits, mins = ref.widths(arrays), [int(x.min()) for x in arrays]
    assert bits == [2, 2, 2]
    codes = [ref.code_of(g[0], mins, bits) for g in got]
    assert codes == sorted(codes) and len(set(codes)) == len(codes)
    # e = v - min + 1 = 2 in every field
    assert ref.code_of((2, 6, 9), mins, bits) == 0b10_10_10


# ---- plan_keys.h, stand-alone ----

def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    return cxx


def _build(tmp_path, name, extra):
    out = str(tmp_path / name)
    src = os.path.join(HERE, "plan_groupn_host_main.cpp")
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                        src, "-o", out] + extra,
                       capture_output=True, text=True)
    return out, r


def _run(prog):
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stderr == ""
    assert re.fullmatch(r"ok \d+\n", r.stdout), r.stdout


def test_decoder_plain(tmp_path):
    prog, r = _build(tmp_path, "plan_groupn_host", [])
    assert r.returncode == 0, r.stderr
    _run(prog)


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _has_sanitizer_runtimes(tmp_path):
    """a trivial program builds and runs with the sanitizers: only their
    absence skips the sanitized test, never a diagnostic about the decoder"""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    out = str(tmp_path / "probe")
    r = subprocess.run([_cxx(), "-std=c++17", str(src), "-o", out] + SAN,
                       capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([out]).returncode == 0


def test_decoder_sanitized(tmp_path):
    if not _has_sanitizer_runtimes(tmp_path):
        pytest.skip("the compiler has no sanitizer runtimes")
    prog, r = _build(tmp_path, "plan_groupn_host_san", SAN)
    assert r.returncode == 0, r.stderr
    _run(prog)


# ---- the fuzz descriptors, on the reference alone ----

def test_fuzz_seed_properties():
    """what the seed of test_gpu_plan_groupn_fuzz.py was chosen for"""
    import test_gpu_plan_groupn_fuzz as fz
    from greengage_amd import engine as ge, plan_group_bits_n
    descs = fz.all_descs()
    assert len(descs) == fz.NDESC == 16
    within = 0
    for d in descs:
        assert len(d["group"]) in (3, 4)
        arrays = [fz.column(d, c) for c in d["group"]]
        bits = ref.widths(arrays)
        rc, lib_bits = plan_group_bits_n([int(a.min()) for a in arrays],
                                         [int(a.max()) for a in arrays])
        assert list(lib_bits) == bits
        assert (rc == OK) == (sum(bits) <= 62)
        within += rc == OK
        # the binding builds every one of them
        dd, _k = ge.build_plan_desc(0, preds=d["preds"], group_cols=d["group"],
                                    aggs=d["aggs"], joins=[
                                        dict(j, table=1 + i) for i, j in
                                        enumerate(ref.strip(d["joins"]))])
        assert dd.ngroup == 2
        assert ge.build_plan_groups(d["group"]).ncols == len(d["group"]) - 2
        if rc == OK:
            assert len(fz.expected(d)[1]) <= 4096
    assert within >= 12
    assert {len(d["group"]) for d in descs} == {3, 4}
    assert sum(fz.has_payload_key(d) for d in descs) >= 5
    assert any(fz.has_left_key(d) for d in descs)
