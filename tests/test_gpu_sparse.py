"""Sparse-key hash-table fallback.

The Q3/Q5 pipelines collapse to dense direct maps when max(key) <=
8x rows (nodeHash.c:450 sizing analog).  These tests feed keys ~1000x
sparser than rows so the guard REJECTS the dense map and the
open-addressing CAS hash tables (k_build_set / k_build_orders /
k_probe_lineitem, q3 stats/hist/collect on DeviceHashTable) run —
asserted bit-exact against the CPU oracle, with the taken path
reported by gg_engine_stats.

The same tables also run through the forced Motion exchange (a world-of-1
RCCL loopback), where the received rows go into the hash tables through
k_insert_orders, and through Q5, whose customer map, supplier table and
orders table all fall back to hash tables on these keys.
"""
import os

import numpy as np
import pytest

import pyoracle

pytestmark = pytest.mark.gpu

SEED = 7


@pytest.fixture(scope="module")
def eng():
    from greengage_amd import Engine
    e = Engine(device=0, n_segments=1, segment_id=0)
    yield e
    e.shutdown()


def make_sparse(ncust=5_000, nord=40_000, lines_per_order=4, stride=1009):
    """TPC-H-shaped tables whose keys are `stride`x sparser than rows
    (stride is prime so key sets stay collision-free)."""
    rng = np.random.default_rng(SEED)
    c_custkey = (np.arange(ncust, dtype=np.int64) + 1) * stride
    c_mktseg = rng.integers(0, 5, ncust).astype(np.uint8)
    o_orderkey = (np.arange(nord, dtype=np.int64) + 1) * stride
    o_custkey = c_custkey[rng.integers(0, ncust, nord)]
    o_orderdate = rng.integers(-2000, 500, nord).astype(np.int32)
    o_prio = rng.integers(0, 2, nord).astype(np.int32)
    nli = nord * lines_per_order
    l_orderkey = np.repeat(o_orderkey, lines_per_order)
    l_shipdate = rng.integers(-2000, 500, nli).astype(np.int32)
    l_price = rng.integers(90100, 10494950, nli).astype(np.int64)
    l_disc = rng.integers(0, 11, nli).astype(np.int64)
    return (c_custkey, c_mktseg, o_orderkey, o_custkey, o_orderdate,
            o_prio, l_orderkey, l_shipdate, l_price, l_disc)


STRIDE = 1009
Q5_LO, Q5_HI, Q5_REGION = -1000, -500, 1


def make_sparse_q5(nsupp=200):
    """make_sparse() plus what Q5 reads: customer and supplier nations in
    0..24, a suppkey per line, suppkeys as sparse as the other keys (so
    every dense guard rejects).  Drawn from a generator of its own, so
    the Q3 tables above stay what they were."""
    (c_ck, _, o_ok, o_ck, o_od, _, l_ok, _, l_pc, l_dc) = make_sparse()
    rng = np.random.default_rng(SEED + 1)
    c_nk = rng.integers(0, 25, len(c_ck)).astype(np.uint8)
    s_sk = (np.arange(nsupp, dtype=np.int64) + 1) * STRIDE
    s_nk = rng.integers(0, 25, nsupp).astype(np.uint8)
    l_sk = s_sk[rng.integers(0, nsupp, len(l_ok))]
    return dict(c_ck=c_ck, c_nk=c_nk, o_ok=o_ok, o_ck=o_ck, o_od=o_od,
                l_ok=l_ok, l_sk=l_sk, l_pc=l_pc, l_dc=l_dc, s_sk=s_sk,
                s_nk=s_nk)


def q5_sparse_expect(t):
    """The oracle's rows over the keys divided by the stride (a bijective
    remap: the joins and the per-nation sums do not see it)."""
    return pyoracle.q5_rows(pyoracle.q5_arrays(
        t["c_ck"] // STRIDE, t["c_nk"], t["o_ok"] // STRIDE,
        t["o_ck"] // STRIDE, t["o_od"], t["l_ok"] // STRIDE,
        t["l_sk"] // STRIDE, t["l_pc"], t["l_dc"], t["s_sk"] // STRIDE,
        t["s_nk"], Q5_REGION, Q5_LO, Q5_HI))


@pytest.fixture(scope="module")
def q3_sparse(eng):
    from greengage_amd.engine import PIPE_Q3
    (c_ck, c_ms, o_ok, o_ck, o_od, o_pr,
     l_ok, l_sd, l_pc, l_dc) = make_sparse()
    cu = eng.register_table("cust_sparse_x", [
        ("custkey", "int64", c_ck), ("mktseg", "char1", c_ms)], len(c_ck))
    od = eng.register_table("ord_sparse_x", [
        ("orderkey", "int64", o_ok), ("custkey", "int64", o_ck),
        ("orderdate", "int32", o_od), ("shippriority", "int32", o_pr)],
        len(o_ok))
    li = eng.register_table("li_sparse_x", [
        ("orderkey", "int64", l_ok), ("shipdate", "int32", l_sd),
        ("price", "dec64", l_pc), ("disc", "dec64", l_dc)], len(l_ok))
    return lambda: eng.compile(PIPE_Q3, lineitem=li, orders=od, customer=cu,
                               cutoff_date=-800, mktsegment=2, limit_k=10)


@pytest.fixture(scope="module")
def q5_sparse(eng):
    """(compile, local rows): the Q5 pipeline over the sparse tables and
    what the local path answers, computed once for both Q5 tests."""
    from greengage_amd.engine import PIPE_Q5
    t = make_sparse_q5()
    li = eng.register_table("li_sparse_q5", [
        ("orderkey", "int64", t["l_ok"]), ("suppkey", "int64", t["l_sk"]),
        ("price", "dec64", t["l_pc"]), ("disc", "dec64", t["l_dc"])],
        len(t["l_ok"]))
    od = eng.register_table("ord_sparse_q5", [
        ("orderkey", "int64", t["o_ok"]), ("custkey", "int64", t["o_ck"]),
        ("orderdate", "int32", t["o_od"])], len(t["o_ok"]))
    cu = eng.register_table("cust_sparse_q5", [
        ("custkey", "int64", t["c_ck"]), ("nationkey", "char1", t["c_nk"])],
        len(t["c_ck"]))
    su = eng.register_table("supp_sparse_q5", [
        ("suppkey", "int64", t["s_sk"]), ("nationkey", "char1", t["s_nk"])],
        len(t["s_sk"]))
    na = eng.register_table("nation_sparse_q5", [
        ("nationkey", "int32", np.arange(25, dtype=np.int32)),
        ("regionkey", "int32", np.array(pyoracle.NATION_REGION, np.int32))],
        25)

    def compile_q5():
        return eng.compile(PIPE_Q5, lineitem=li, orders=od, customer=cu,
                           supplier=su, nation=na, cutoff_date=Q5_LO,
                           cutoff_hi=Q5_HI, regionkey=Q5_REGION)
    p = compile_q5()
    return compile_q5, p, eng.execute_q5(p), q5_sparse_expect(t)


@pytest.fixture(scope="module")
def comm(eng):
    """RCCL world of 1 on the module's engine, for the forced exchange;
    the engine's shutdown tears it down."""
    eng.comm_init(eng.comm_id())


def path_names(eng, p):
    return {s["name"] for s in eng.stats(p)}


def test_q3_sparse_keys_forced_exchange(eng, q3_sparse, comm):
    """Sparse keys through both redistribute legs: the received orders
    are inserted by k_insert_orders, bit for bit the fused result."""
    rows_f, hdr_f = eng.execute_q3(q3_sparse())
    assert hdr_f["n_out"] == 10
    os.environ["GG_FORCE_EXCHANGE"] = "1"
    try:
        p_x = q3_sparse()
        rows_x, hdr_x = eng.execute_q3(p_x)
        # steady state (scratch reuse, cached sizing): same again
        rows_x2, hdr_x2 = eng.execute_q3(p_x)
    finally:
        del os.environ["GG_FORCE_EXCHANGE"]
    assert hdr_x == hdr_f and rows_x == rows_f
    assert hdr_x2 == hdr_f and rows_x2 == rows_f
    names = path_names(eng, p_x)
    assert {"path_cust_hash", "path_orders_hash",
            "orders_exchange"} <= names, names


def test_q5_sparse_keys_hash_fallback(eng, q5_sparse):
    _, p, rows, expect = q5_sparse
    assert len(expect) >= 2
    assert [(r["nationkey"], r["count"], r["revenue4"]) for r in rows] == \
           [(r["nationkey"], r["count"], r["revenue4"]) for r in expect]
    names = path_names(eng, p)
    assert {"path_cust_hash", "path_orders_hash"} <= names, names
    assert "path_cust_dense" not in names
    assert "path_orders_dense" not in names


def test_q5_sparse_keys_forced_exchange(eng, q5_sparse, comm):
    compile_q5, _, rows_f, _ = q5_sparse
    os.environ["GG_FORCE_EXCHANGE"] = "1"
    try:
        p_x = compile_q5()
        rows_x = eng.execute_q5(p_x)
        rows_x2 = eng.execute_q5(p_x)
    finally:
        del os.environ["GG_FORCE_EXCHANGE"]
    assert rows_x == rows_f
    assert rows_x2 == rows_f
    names = path_names(eng, p_x)
    assert {"path_cust_hash", "path_orders_hash",
            "orders_exchange"} <= names, names


def test_q3_sparse_keys_hash_fallback(eng):
    from greengage_amd.engine import PIPE_Q3
    (c_ck, c_ms, o_ok, o_ck, o_od, o_pr,
     l_ok, l_sd, l_pc, l_dc) = make_sparse()

    cu = eng.register_table("cust_sparse", [
        ("custkey", "int64", c_ck), ("mktseg", "char1", c_ms)], len(c_ck))
    od = eng.register_table("ord_sparse", [
        ("orderkey", "int64", o_ok), ("custkey", "int64", o_ck),
        ("orderdate", "int32", o_od), ("shippriority", "int32", o_pr)],
        len(o_ok))
    li = eng.register_table("li_sparse", [
        ("orderkey", "int64", l_ok), ("shipdate", "int32", l_sd),
        ("price", "dec64", l_pc), ("disc", "dec64", l_dc)], len(l_ok))

    cutoff = -800
    p = eng.compile(PIPE_Q3, lineitem=li, orders=od, customer=cu,
                    cutoff_date=cutoff, mktsegment=2, limit_k=10)
    rows, hdr = eng.execute_q3(p)

    # the guard must have rejected the dense map on BOTH sides
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    assert "path_cust_hash" in paths, paths
    assert "path_orders_hash" in paths, paths
    assert "path_cust_bitmap" not in paths
    assert "path_orders_dense" not in paths

    # The CPU oracle's Q3 uses dense key arrays internally, so feed it
    # a bijectively remapped (key/stride) copy — join/group semantics
    # and revenue sums are invariant under the remap; top-k orderkeys
    # map back by *stride.  group_checksum hashes the raw orderkey
    # values so it is not comparable across the remap (the dense-path
    # control test below pins it instead).
    stride = 1009
    topk, res = pyoracle.q3_arrays(
        c_ck // stride, c_ms, 2, o_ok // stride, o_ck // stride,
        o_od, o_pr, l_ok // stride, l_sd, l_pc, l_dc, cutoff)
    assert hdr["n_groups"] == res["n_groups"]
    assert hdr["n_join_rows"] == res["n_join_rows"]
    assert hdr["rev_sum4"] == res["rev_sum4"]
    assert [(r["orderkey"], r["revenue4"], r["orderdate"],
             r["shippriority"]) for r in rows] == \
           [(r["orderkey"] * stride, r["revenue4"], r["orderdate"],
             r["shippriority"]) for r in topk]


def test_q3_dense_keys_report_dense_path(eng):
    """Control: dbgen-shaped dense keys must keep the dense map (and
    still match the oracle), so the guard is pinned from both sides."""
    from greengage_amd import PGDate
    from greengage_amd.engine import PIPE_Q3
    li = eng.register_synth("lineitem", seed=42, sf=1)
    od = eng.register_synth("orders", seed=42, sf=1)
    cu = eng.register_synth("customer", seed=42, sf=1)
    cutoff = PGDate("1995-03-15")
    p = eng.compile(PIPE_Q3, lineitem=li, orders=od, customer=cu,
                    cutoff_date=cutoff, mktsegment=2, limit_k=10)
    rows, hdr = eng.execute_q3(p)
    paths = {s["name"] for s in eng.stats(p) if s["name"].startswith("path")}
    assert "path_cust_bitmap" in paths, paths
    assert "path_orders_dense" in paths, paths
    _, res = pyoracle.q3_synth(42, 1, cutoff, k=10)
    assert hdr["n_groups"] == res["n_groups"]
    assert hdr["group_checksum"] == res["group_checksum"]
