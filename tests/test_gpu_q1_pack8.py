"""Q1 over the 8 B tier of the packed companion ("Packed Q1
companion"): one u64 per row when the table's own ranges fit 64 bits.  The
tables here are drawn so that the widths sum to exactly 64 (qty 16 bits,
price 25, disc 0..100 = 7, tax 8, shipdate span 31 = 5, code 3), all six
groups present.  The reference is a Python big-int evaluation; the wide
kernel (GG_Q1_PACK=0) and the 12 B tier (GG_Q1_PACK=12 at compile, over a
separately registered table) must give the same.  Every case that expects a
tier asserts the path_q1_* stat rows and the bytes accounted."""
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
SD_LO, SD_SPAN = 9000, 31
PBITS = 25


@pytest.fixture(scope="module")
def eng():
    from greengage_amd import Engine
    e = Engine(device=0, n_segments=1, segment_id=0)
    yield e
    e.shutdown()


def make_table(n, seed, pbits=PBITS, sd_span=SD_SPAN):
    """n >= 12 rows, every field's maximum and minimum present, so the
    widths are 16 + pbits + 7 + 8 + bits(sd_span) + 3."""
    r = np.random.default_rng(seed)
    t = {
        "qty": r.integers(0, 65536, n, dtype=np.int64),
        "price": r.integers(0, 2**pbits, n, dtype=np.int64),
        "disc": r.integers(0, 101, n, dtype=np.int64),
        "tax": r.integers(0, 256, n, dtype=np.int64),
        "shipdate": r.integers(SD_LO, SD_LO + sd_span + 1, n,
                               dtype=np.int64).astype(np.int32),
        "rflag": np.array(RF, np.uint8)[r.integers(0, 3, n)],
        "lstatus": np.array(LS, np.uint8)[r.integers(0, 2, n)],
    }
    for i in range(6):                  # every group
        t["rflag"][i] = RF[i // 2]
        t["lstatus"][i] = LS[i % 2]
    # a row with every field at its maximum, one with every field at zero
    t["qty"][6], t["price"][6], t["disc"][6], t["tax"][6] = \
        65535, 2**pbits - 1, 100, 255
    t["shipdate"][6] = SD_LO + sd_span
    t["qty"][7] = t["price"][7] = t["disc"][7] = t["tax"][7] = 0
    t["shipdate"][7] = SD_LO
    return t


def width(t):
    span = int(t["shipdate"].max()) - int(t["shipdate"].min())
    return sum(int(t[k].max()).bit_length()
               for k in ("qty", "price", "disc", "tax")) + \
        span.bit_length() + 3


def register(eng, name, t):
    n = len(t["qty"])
    cols = [("orderkey", "int64", np.arange(n, dtype=np.int64)),
            ("qty", "dec64", t["qty"]), ("price", "dec64", t["price"]),
            ("disc", "dec64", t["disc"]), ("tax", "dec64", t["tax"]),
            ("shipdate", "int32", t["shipdate"]),
            ("rflag", "char1", t["rflag"]),
            ("lstatus", "char1", t["lstatus"])]
    return eng.register_table(name, cols, n)


def drop(eng, h):
    from greengage_amd.engine import lib
    assert lib().gg_engine_drop_table(h) == 0


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


def run(eng, h, cutoff, monkeypatch, pack=None, tier=None):
    """compile + execute under GG_Q1_PACK=pack (None: unset); tier 8, 12 or
    38 (wide) asserts the stat rows and the bytes of that path"""
    from greengage_amd.engine import PIPE_Q1
    if pack is None:
        monkeypatch.delenv("GG_Q1_PACK", raising=False)
    else:
        monkeypatch.setenv("GG_Q1_PACK", pack)
    try:
        p = eng.compile(PIPE_Q1, lineitem=h, cutoff_date=cutoff)
        got = eng.execute_q1(p)
    finally:
        monkeypatch.delenv("GG_Q1_PACK", raising=False)
    st = {s["name"]: s for s in eng.stats(p)}
    if tier:
        n = st["q1_agg"]["rows_in"]
        assert ("path_q1_packed8" in st) == (tier == 8)
        assert ("path_q1_packed" in st) == (tier in (8, 12))
        assert ("path_q1_wide" in st) == (tier == 38)
        for name in ("path_q1_packed8", "path_q1_packed", "path_q1_wide"):
            assert st.get(name, {"launches": 1})["launches"] == 1
        assert st["q1_agg"]["hbm_bytes_algorithmic"] == tier * n
        if "q1_pack_build" in st:
            assert st["q1_pack_build"]["launches"] == 1
            assert st["q1_pack_build"]["hbm_bytes_algorithmic"] == \
                (38 + tier) * n
    return got, st


# ---- 1. sizes and tails, against the reference, wide and the 12 B tier ----

@pytest.mark.parametrize("n", [1024, 1025, 1027, 4099, 100003])
def test_sizes_and_tails(eng, monkeypatch, n):
    t = make_table(n, 2000 + n)
    assert width(t) == 64
    cutoff = SD_LO + 20
    ref = reference(t, cutoff)
    assert len(ref) == 6
    h8 = register(eng, "p8_%d" % n, t)
    h12 = register(eng, "p12_%d" % n, t)
    # the wide run first: it must not find (or build) a companion
    wide, st = run(eng, h8, cutoff, monkeypatch, pack="0", tier=38)
    assert "q1_pack_build" not in st
    got8, st = run(eng, h8, cutoff, monkeypatch, tier=8)
    assert st["q1_agg"]["rows_in"] == n
    assert st["q1_agg"]["hbm_bytes_algorithmic"] == 8 * n
    assert st["q1_pack_build"]["launches"] == 1
    got12, st = run(eng, h12, cutoff, monkeypatch, pack="12", tier=12)
    assert st["q1_pack_build"]["launches"] == 1
    same(got8, ref)
    same(got12, ref)
    same(wide, ref)
    assert got8 == got12 == wide
    # companions exist now and are used as they are: GG_Q1_PACK=12 does not
    # demote an 8 B one, its absence does not promote a 12 B one, and
    # GG_Q1_PACK=0 still forces the wide kernel
    again, st = run(eng, h8, cutoff, monkeypatch, pack="12", tier=8)
    assert "q1_pack_build" not in st and again == got8
    again, st = run(eng, h12, cutoff, monkeypatch, tier=12)
    assert "q1_pack_build" not in st and again == got8
    again, _ = run(eng, h8, cutoff, monkeypatch, pack="0", tier=38)
    assert again == got8
    drop(eng, h8)
    drop(eng, h12)


# ---- 1b. both accumulation forms: folded count/disc/qty word, six adds ----

@pytest.mark.parametrize("grid", [None, "1"])
def test_folded_and_six_add_forms(eng, monkeypatch, grid):
    """On the default grid (196 blocks) a replica sees 35 rows and count,
    sum(disc) and sum(qty) share one LDS word; one forced block gives a
    replica 6275 rows, the proof fails and the kernel keeps six adds
    (test_q1_pack8_cpu.py pins both decisions).  A lane of the single block
    takes 196 quads, one of the last iteration's lanes an odd number."""
    n = 200_003
    t = make_table(n, 99)
    assert width(t) == 64
    cutoff = SD_LO + 25
    if grid:
        monkeypatch.setenv("GG_Q1_GRID", grid)
    h = register(eng, "forms8", t)
    got, _ = run(eng, h, cutoff, monkeypatch, tier=8)
    same(got, reference(t, cutoff))
    drop(eng, h)


# ---- 2. what does not fit stays on the 12 B tier ----

def test_65_bits_and_1023_rows_take_the_12_byte_tier(eng, monkeypatch):
    cutoff = SD_LO + 20
    wide65 = make_table(1025, 41, pbits=PBITS + 1)
    assert width(wide65) == 65
    short = make_table(1023, 42)
    assert width(short) == 64
    for name, t in (("w65", wide65), ("n1023", short)):
        h = register(eng, name, t)
        got, st = run(eng, h, cutoff, monkeypatch, tier=12)
        assert st["q1_pack_build"]["launches"] == 1
        same(got, reference(t, cutoff))
        drop(eng, h)


# ---- 3. cutoff edges over one companion ----

def test_cutoff_edges_share_one_companion(eng, monkeypatch):
    t = make_table(5003, 7)
    sd_min, sd_max = int(t["shipdate"].min()), int(t["shipdate"].max())
    assert (sd_min, sd_max) == (SD_LO, SD_LO + SD_SPAN) and width(t) == 64
    h = register(eng, "cut8", t)
    builds = 0
    for cutoff in (sd_min - 1, sd_min, (sd_min + sd_max) // 2, sd_max,
                   sd_max + 1, INT32_MIN, INT32_MAX):
        got, st = run(eng, h, cutoff, monkeypatch)
        assert st["path_q1_packed8"]["launches"] == 1
        assert st["path_q1_packed"]["launches"] == 1
        builds += st.get("q1_pack_build", {"launches": 0})["launches"]
        same(got, reference(t, cutoff))
    assert builds == 1
    assert reference(t, sd_min - 1) == [] and reference(t, sd_min) != []
    assert reference(t, sd_max) == reference(t, INT32_MAX)
    assert reference(t, sd_max - 1) != reference(t, sd_max)
    drop(eng, h)


# ---- 4. bad flag byte ----

@pytest.mark.parametrize("row", [10, 1024])     # a whole quad, the tail
def test_bad_flag_byte(eng, monkeypatch, row):
    from greengage_amd.engine import EngineError
    t = make_table(1025, 77)
    late = SD_LO + SD_SPAN
    t["shipdate"][t["shipdate"] == late] = late - 1
    t["shipdate"][row] = late           # the only row of the last day
    t["rflag"][row] = ord("X")
    assert width(t) == 64
    h = register(eng, "badflag8", t)
    # the cutoff filters the row out: nothing raised, the reference answer
    got, _ = run(eng, h, late - 1, monkeypatch, tier=8)
    ok = dict(t)
    ok["rflag"] = t["rflag"].copy()
    ok["rflag"][row] = ord("A")         # filtered out, so its group is moot
    same(got, reference(ok, late - 1))
    # the row passes: the error surfaces
    with pytest.raises(EngineError):
        run(eng, h, late, monkeypatch)
    drop(eng, h)


# ---- 5. lifetime ----

def test_drop_then_register_same_size(eng, monkeypatch):
    a = make_table(4099, 5)
    b = make_table(4099, 6)
    cutoff = SD_LO + 15
    ha = register(eng, "life8_a", a)
    got, _ = run(eng, ha, cutoff, monkeypatch, tier=8)
    same(got, reference(a, cutoff))
    drop(eng, ha)
    hb = register(eng, "life8_b", b)
    got, st = run(eng, hb, cutoff, monkeypatch, tier=8)
    assert st["q1_pack_build"]["launches"] == 1
    same(got, reference(b, cutoff))
    assert reference(a, cutoff) != reference(b, cutoff)
    drop(eng, hb)


# ---- 6. SF1 ----

def test_sf1_takes_the_8_byte_tier(eng, monkeypatch):
    from greengage_amd import PGDate
    cutoff = PGDate("1998-08-15")
    li = eng.register_synth("lineitem", seed=42, sf=1)
    got, st = run(eng, li, cutoff, monkeypatch, tier=8)
    assert st["q1_agg"]["rows_in"] == 6_000_000
    expect = [g for g in pyoracle.q1_synth(42, 1, cutoff) if g["count"]]
    assert len(got) == len(expect)
    for g, exp in zip(got, expect):
        for k in KEYS:
            assert g[k] == exp[k], k
