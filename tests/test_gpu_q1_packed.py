"""Q1 over the packed companion ("Packed Q1 companion"): the
12 B/row path against a Python big-int evaluation of the six sums per group
and against the wide kernel (GG_Q1_PACK=0), over sizes and tails, cutoff
edges, the 128-bit carry, every eligibility fallback, bad flag bytes, table
lifetime, and the SF1 synthetic table.  Every case that expects a path also
asserts the path_q1_* stat row."""
import numpy as np
import pytest

import pyoracle

pytestmark = pytest.mark.gpu

KEYS = ("count", "sum_qty_c", "sum_base_c", "sum_dcol_c", "sum_disc4",
        "sum_charge6")
RF = (ord("A"), ord("N"), ord("R"))
LS = (ord("F"), ord("O"))
INT32_MAX = 2**31 - 1
INT32_MIN = -2**31


@pytest.fixture(scope="module")
def eng():
    from greengage_amd import Engine
    e = Engine(device=0, n_segments=1, segment_id=0)
    yield e
    e.shutdown()


def make_table(n, seed, sd_lo=9000, sd_span=65535):
    """n rows uniform over the full eligible ranges, all six groups."""
    r = np.random.default_rng(seed)
    t = {
        "qty": r.integers(0, 65536, n, dtype=np.int64),
        "price": r.integers(0, 2**32, n, dtype=np.int64),
        "disc": r.integers(0, 101, n, dtype=np.int64),
        "tax": r.integers(0, 256, n, dtype=np.int64),
        "shipdate": r.integers(sd_lo, sd_lo + sd_span + 1, n,
                               dtype=np.int64).astype(np.int32),
        "rflag": np.array(RF, np.uint8)[r.integers(0, 3, n)],
        "lstatus": np.array(LS, np.uint8)[r.integers(0, 2, n)],
    }
    # every group at the front, so that even tiny tables hold as many as fit
    for i in range(min(n, 6)):
        t["rflag"][i] = RF[i // 2]
        t["lstatus"][i] = LS[i % 2]
    return t


def register(eng, name, t):
    n = len(t["qty"])
    cols = [("orderkey", "int64", np.arange(n, dtype=np.int64)),
            ("qty", "dec64", t["qty"]), ("price", "dec64", t["price"]),
            ("disc", "dec64", t["disc"]), ("tax", "dec64", t["tax"]),
            ("shipdate", "int32", t["shipdate"]),
            ("rflag", "char1", t["rflag"]),
            ("lstatus", "char1", t["lstatus"])]
    return eng.register_table(name, cols, n)


def reference(t, cutoff):
    """The six sums per group in Python integers, in the engine's group
    order (A,F) (A,O) (N,F) (N,O) (R,F) (R,O); empty groups left out."""
    out = []
    keep = t["shipdate"].astype(np.int64) <= cutoff
    for rf in RF:
        for ls in LS:
            m = keep & (t["rflag"] == rf) & (t["lstatus"] == ls)
            if not m.any():
                continue
            q = [int(x) for x in t["qty"][m]]
            p = [int(x) for x in t["price"][m]]
            d = [int(x) for x in t["disc"][m]]
            x = [int(x) for x in t["tax"][m]]
            d4 = [pi * (100 - di) for pi, di in zip(p, d)]
            out.append({
                "returnflag": chr(rf), "linestatus": chr(ls),
                "count": len(q), "sum_qty_c": sum(q), "sum_base_c": sum(p),
                "sum_dcol_c": sum(d), "sum_disc4": sum(d4),
                "sum_charge6": sum(v * (100 + xi)
                                   for v, xi in zip(d4, x)),
            })
    return out


def same(got, ref):
    assert [(g["returnflag"], g["linestatus"]) for g in got] == \
        [(g["returnflag"], g["linestatus"]) for g in ref]
    for g, r in zip(got, ref):
        for k in KEYS:
            assert g[k] == r[k], (g["returnflag"], g["linestatus"], k)


def stat(eng, p):
    return {s["name"]: s for s in eng.stats(p)}


def run(eng, t, cutoff, monkeypatch, pack, path=None):
    """compile + execute over a registered table handle under GG_Q1_PACK"""
    from greengage_amd.engine import PIPE_Q1
    if pack:
        monkeypatch.delenv("GG_Q1_PACK", raising=False)
    else:
        monkeypatch.setenv("GG_Q1_PACK", "0")
    p = eng.compile(PIPE_Q1, lineitem=t, cutoff_date=cutoff)
    got = eng.execute_q1(p)
    st = stat(eng, p)
    if path:
        other = "wide" if path == "packed" else "packed"
        assert st["path_q1_" + path]["launches"] == 1
        assert "path_q1_" + other not in st
    monkeypatch.delenv("GG_Q1_PACK", raising=False)
    return got, st


# ---- 1. sizes and tails ----

@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 1025, 4099, 100003])
def test_sizes_and_tails(eng, monkeypatch, n):
    t = make_table(n, 1000 + n)
    cutoff = 9000 + 40000
    ref = reference(t, cutoff)
    if n >= 6:
        assert len(reference(t, INT32_MAX)) == 6
    # the wide run first: it must not find (or build) a companion
    h = register(eng, "sz%d" % n, t)
    wide, st = run(eng, h, cutoff, monkeypatch, pack=False, path="wide")
    assert "q1_pack_build" not in st
    packed, st = run(eng, h, cutoff, monkeypatch, pack=True, path="packed")
    assert st["q1_pack_build"]["launches"] == 1
    assert st["q1_agg"]["hbm_bytes_algorithmic"] == 12 * n
    same(packed, ref)
    same(wide, ref)
    assert packed == wide
    # a companion exists now; GG_Q1_PACK=0 still forces the wide kernel
    again, _ = run(eng, h, cutoff, monkeypatch, pack=False, path="wide")
    assert again == wide
    eng_drop(eng, h)


def eng_drop(eng, h):
    from greengage_amd.engine import lib
    assert lib().gg_engine_drop_table(h) == 0


# ---- 2. cutoff edges ----

def test_cutoff_edges_share_one_companion(eng, monkeypatch):
    from greengage_amd.engine import PIPE_Q1
    monkeypatch.delenv("GG_Q1_PACK", raising=False)
    t = make_table(5003, 7, sd_lo=-30000, sd_span=65535)
    t["shipdate"][4000] = -30000            # both ends of the widest span
    t["shipdate"][17] = -30000 + 65535
    sd_min, sd_max = int(t["shipdate"].min()), int(t["shipdate"].max())
    assert sd_max - sd_min == 65535
    h = register(eng, "cut", t)
    builds = 0
    for cutoff in (sd_min - 1, sd_min, (sd_min + sd_max) // 2, sd_max,
                   sd_max + 1, INT32_MAX, INT32_MIN):
        p = eng.compile(PIPE_Q1, lineitem=h, cutoff_date=cutoff)
        got = eng.execute_q1(p)
        st = stat(eng, p)
        assert st["path_q1_packed"]["launches"] == 1
        builds += st.get("q1_pack_build", {"launches": 0})["launches"]
        same(got, reference(t, cutoff))
    assert builds == 1
    assert reference(t, sd_min - 1) == [] and reference(t, sd_min) != []
    eng_drop(eng, h)


# ---- 3. 128-bit carry ----

@pytest.mark.parametrize("grid", [None, "1"])
def test_charge_carries_past_64_bits(eng, monkeypatch, grid):
    n = 200_000
    t = {"qty": np.full(n, 65535, np.int64),
         "price": np.full(n, 2**32 - 1, np.int64),
         "disc": np.zeros(n, np.int64), "tax": np.full(n, 255, np.int64),
         "shipdate": np.full(n, 10, np.int32),
         "rflag": np.full(n, ord("N"), np.uint8),
         "lstatus": np.full(n, ord("O"), np.uint8)}
    ref = reference(t, 10)
    assert ref[0]["sum_charge6"] == n * (2**32 - 1) * 100 * 355 > 2**64
    if grid:
        monkeypatch.setenv("GG_Q1_GRID", grid)
    h = register(eng, "carry", t)
    # exact either way: the grid floor raises a forced grid of 1, or the
    # host refuses the packed path; which of the two is not prescribed
    got, st = run(eng, h, 10, monkeypatch, pack=True)
    assert ("path_q1_packed" in st) != ("path_q1_wide" in st)
    same(got, ref)
    assert got[0]["sum_charge6"] >> 64 == ref[0]["sum_charge6"] >> 64 == 1
    eng_drop(eng, h)


# ---- 4. fallbacks ----

def _break(t, what):
    if what == "negative qty":
        t["qty"][5] = -1
    elif what == "price 2^32":
        t["price"][5] = 2**32
    elif what == "qty 65536":
        t["qty"][5] = 65536
    elif what == "disc 101":
        # 100 - disc goes negative; a small price keeps every partial sum
        # of the wide kernel non-negative, where its u64 words are exact
        t["disc"][5] = 101
        t["price"][5] = 1000
    elif what == "tax 256":
        t["tax"][5] = 256
    elif what == "shipdate span 65536":
        t["shipdate"][5] = 9000
        t["shipdate"][6] = 9000 + 65536
    return t


@pytest.mark.parametrize("what", ["negative qty", "price 2^32", "qty 65536",
                                  "disc 101", "tax 256",
                                  "shipdate span 65536"])
def test_ineligible_table_runs_wide(eng, monkeypatch, what):
    t = _break(make_table(1025, 31, sd_span=60000), what)
    cutoff = 9000 + 70000
    h = register(eng, "fb", t)
    got, st = run(eng, h, cutoff, monkeypatch, pack=True, path="wide")
    assert "q1_pack_build" not in st
    assert st["q1_agg"]["hbm_bytes_algorithmic"] == 38 * 1025
    same(got, reference(t, cutoff))
    eng_drop(eng, h)


# ---- 5. bad flag byte ----

@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("row", [2, 1024])      # a whole quad, the tail
def test_bad_flag_byte(eng, monkeypatch, pack, row):
    from greengage_amd.engine import EngineError
    t = make_table(1025, 77, sd_span=1000)
    t["shipdate"][row] = 9000 + 5000
    t["rflag"][row] = ord("X")
    path = "packed" if pack else "wide"
    h = register(eng, "badflag", t)
    # the cutoff filters the row out: nothing raised, the reference answer
    got, _ = run(eng, h, 9000 + 4999, monkeypatch, pack, path=path)
    ok = dict(t)
    ok["rflag"] = t["rflag"].copy()
    ok["rflag"][row] = ord("A")     # filtered out, so its group is moot
    same(got, reference(ok, 9000 + 4999))
    # the row passes: the error surfaces on both paths
    with pytest.raises(EngineError):
        run(eng, h, 9000 + 5000, monkeypatch, pack)
    monkeypatch.delenv("GG_Q1_PACK", raising=False)
    eng_drop(eng, h)


# ---- 6. lifetime ----

def test_drop_then_register_same_size(eng, monkeypatch):
    a = make_table(4099, 5)
    b = make_table(4099, 6)
    cutoff = 9000 + 30000
    ha = register(eng, "life_a", a)
    got, _ = run(eng, ha, cutoff, monkeypatch, pack=True, path="packed")
    same(got, reference(a, cutoff))
    eng_drop(eng, ha)
    hb = register(eng, "life_b", b)
    got, st = run(eng, hb, cutoff, monkeypatch, pack=True, path="packed")
    assert st["q1_pack_build"]["launches"] == 1
    same(got, reference(b, cutoff))
    assert reference(a, cutoff) != reference(b, cutoff)
    eng_drop(eng, hb)


# ---- 7. SF1 ----

def test_sf1_packed_wide_oracle(eng, monkeypatch):
    from greengage_amd import PGDate
    cutoff = PGDate("1998-08-15")
    li = eng.register_synth("lineitem", seed=42, sf=1)
    packed, st = run(eng, li, cutoff, monkeypatch, pack=True, path="packed")
    assert st["q1_agg"]["rows_in"] == 6_000_000
    wide, _ = run(eng, li, cutoff, monkeypatch, pack=False, path="wide")
    expect = [g for g in pyoracle.q1_synth(42, 1, cutoff) if g["count"]]
    assert packed == wide
    assert len(packed) == len(expect)
    for got, exp in zip(packed, expect):
        for k in KEYS:
            assert got[k] == exp[k], k
