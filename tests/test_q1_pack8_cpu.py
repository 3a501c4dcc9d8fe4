"""Host arithmetic of the 8 B tier of the packed Q1 companion, without a
GPU: the functions of greengage_amd/csrc/q1_pack.h compiled into a
stand-alone program (q1_pack8_host_main.cpp, its own main, built with the
address and undefined-behaviour sanitizers where the compiler has their
runtimes) and asked about the width rule, the row floor, the layout's shifts
and masks, the round trip of boundary rows, the cutoff clamp, the grid and
the proof that lets count, sum(disc) and sum(qty) share one LDS word.
Expectations are computed here in Python integers.
"""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
MIN_ROWS = 1024
ORDER = ("qmin", "qmax", "pmin", "pmax", "dmin", "dmax", "tmin", "tmax",
         "sdmin", "sdmax")
# include/gg_gen.h and dbgen: 13 + 24 + 4 + 4 + 12 + 3 bits
TPCH = dict(qmin=100, qmax=5100, pmin=90000, pmax=10_000_000, dmin=0, dmax=10,
            tmin=0, tmax=8, sdmin=-2921, sdmax=-2921 + 2530)
# exactly 64: 16 + 25 + 7 + 8 + 5 + 3
W64 = dict(qmin=0, qmax=65535, pmin=0, pmax=2**25 - 1, dmin=0, dmax=100,
           tmin=0, tmax=255, sdmin=9000, sdmax=9031)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("q1pack8") / "q1_pack8_host")
    src = os.path.join(HERE, "q1_pack8_host_main.cpp")
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


def rng(v):
    return " ".join(str(v[k]) for k in ORDER)


def widths(v):
    """(shipdate, disc, tax, qty, price) bit lengths, in layout order"""
    return ((v["sdmax"] - v["sdmin"]).bit_length(), v["dmax"].bit_length(),
            v["tmax"].bit_length(), v["qmax"].bit_length(),
            v["pmax"].bit_length())


def width_sum(v):
    return sum(widths(v)) + 3


def layout(v):
    """name -> (shift, mask), as the header documents it: shipdate offset
    at bit 0, then code, disc, tax, qty, price on top"""
    sb, db, tb, qb, pb = widths(v)
    out, at = {}, 0
    for name, b in (("sd", sb), ("code", 3), ("d", db), ("t", tb), ("q", qb),
                    ("p", pb)):
        out[name] = (at, (1 << b) - 1)
        at += b
    return out, at


def test_width_sum_and_tpch_is_60_bits(prog):
    cases = [TPCH, W64, dict(W64, pmax=2**25), dict(W64, sdmax=9032),
             dict(W64, qmax=0), dict(W64, dmax=0, tmax=0),
             dict(W64, sdmax=9000), dict(W64, pmax=0),
             dict(qmin=0, qmax=0, pmin=0, pmax=0, dmin=0, dmax=0, tmin=0,
                  tmax=0, sdmin=7, sdmax=7),
             dict(W64, pmax=2**32 - 1, sdmax=9000 + 65535)]
    got = prog(["W " + rng(v) for v in cases])
    assert got == [str(width_sum(v)) for v in cases]
    assert width_sum(TPCH) == 60 and widths(TPCH) == (12, 4, 4, 13, 24)
    assert width_sum(W64) == 64
    assert width_sum(cases[-1]) == 82            # the widest 12 B table


def test_eligibility_64_65_and_row_floor(prog):
    cases = [
        (MIN_ROWS, W64, 1),
        (MIN_ROWS, dict(W64, pmax=2**25), 0),           # 65 bits
        (MIN_ROWS, dict(W64, sdmax=9032), 0),           # 65 bits
        (MIN_ROWS, dict(W64, pmax=2**25 - 2), 1),
        (MIN_ROWS - 1, W64, 0), (MIN_ROWS, W64, 1), (MIN_ROWS + 1, W64, 1),
        (1, TPCH, 0), (0, TPCH, 0), (6_000_000, TPCH, 1),
        (600_000_000, TPCH, 1),
        # zero-width fields
        (5000, dict(W64, qmax=0, dmax=0, tmax=0, sdmax=9000, pmax=0), 1),
        (5000, dict(W64, pmax=2**32 - 1, dmax=0, qmax=2**13 - 1), 1),  # 61
        # fails q1_pack_eligible: never eligible, however narrow
        (5000, dict(TPCH, qmin=-1), 0), (5000, dict(TPCH, pmin=-1), 0),
        (5000, dict(TPCH, dmin=-1), 0), (5000, dict(TPCH, tmin=-1), 0),
        (5000, dict(TPCH, dmax=101), 0), (5000, dict(TPCH, tmax=256), 0),
        (5000, dict(TPCH, qmax=65536), 0), (5000, dict(TPCH, pmax=2**32), 0),
        (5000, dict(TPCH, sdmin=0, sdmax=65536), 0),
        (5000, dict(TPCH, sdmin=INT32_MIN, sdmax=INT32_MAX), 0),
        (5000, dict(TPCH, qmin=-2**63, qmax=2**63 - 1), 0),
        # the one-row table of the 12 B tier's size test: 61 bits, 1 row
        (1, dict(W64, pmax=2**32 - 1, qmax=2**11 - 1, dmax=100, tmax=255,
                 sdmax=9000), 0),
    ]
    got = prog(["E %d %s" % (n, rng(v)) for n, v, _ in cases])
    assert got == [str(e) for _, _, e in cases]
    for n, v, e in cases[:13]:
        assert e == int(n >= MIN_ROWS and width_sum(v) <= 64)


LAYOUT_CASES = [
    TPCH, W64,
    dict(W64, qmax=0), dict(W64, pmax=0), dict(W64, dmax=0),
    dict(W64, tmax=0), dict(W64, sdmax=9000),
    dict(W64, qmax=0, pmax=0, dmax=0, tmax=0, sdmax=9000),      # 3 bits
    dict(W64, pmax=2**32 - 1, qmax=1, dmax=1, tmax=1, sdmax=9001),
    dict(W64, pmax=7, qmax=65535, dmax=100, tmax=255,
         sdmin=INT32_MIN, sdmax=INT32_MIN + 65535),     # price shift 50
    dict(W64, pmax=2**14 - 1, sdmin=INT32_MAX - 65535, sdmax=INT32_MAX),
]


def test_layout_shifts_and_masks(prog):
    got = prog(["L " + rng(v) for v in LAYOUT_CASES])
    for v, line in zip(LAYOUT_CASES, got):
        (sd_mask, code_shift, d_shift, d_mask, t_shift, t_mask, q_shift,
         q_mask, p_shift, p_mask, bits) = (int(x) for x in line.split())
        lay, total = layout(v)
        assert total == width_sum(v) <= 64
        assert (0, sd_mask) == lay["sd"]
        assert code_shift == lay["code"][0]
        assert (d_shift, d_mask) == lay["d"]
        assert (t_shift, t_mask) == lay["t"]
        assert (q_shift, q_mask) == lay["q"]
        assert (p_shift, p_mask) == lay["p"]
        assert bits == total
        # no shift reaches 64, a zero-width field has mask 0, and the date
        # offset, the code and disc sit inside the low dword
        assert max(code_shift, d_shift, t_shift, q_shift, p_shift) < 64
        for name, mx in (("d", "dmax"), ("t", "tmax"), ("q", "qmax"),
                         ("p", "pmax")):
            assert (lay[name][1] == 0) == (v[mx] == 0)
        assert (sd_mask == 0) == (v["sdmax"] == v["sdmin"])
        assert code_shift + 3 <= 32
        assert d_shift + d_mask.bit_length() <= 32


def test_boundary_rows_round_trip(prog):
    lines, expect = [], []
    for v in LAYOUT_CASES:
        lay, _ = layout(v)
        ends = [(0, v["sdmax"] - v["sdmin"]), (0, 5, 7), (0, v["dmax"]),
                (0, v["tmax"]), (0, v["qmax"]), (0, v["pmax"])]
        rows = set(itertools.product(*[sorted(set(e)) for e in ends]))
        # the masks' own maxima too (every bit of a field set)
        rows.add(tuple(lay[k][1] for k in ("sd", "code", "d", "t", "q", "p")))
        for sd, code, d, t, q, p in sorted(rows):
            word = 0
            for name, val in (("sd", sd), ("code", code), ("d", d), ("t", t),
                              ("q", q), ("p", p)):
                sh, mask = lay[name]
                assert val <= mask
                word |= val << sh
            assert word < 2**64
            lines.append("P %s %d %d %d %d %d %d" % (rng(v), sd, code, d, t,
                                                     q, p))
            expect.append("%d %d %d %d %d %d %d" % (word, sd, code, d, t, q,
                                                    p))
    assert prog(lines) == expect
    # a full 64-bit table with every field at its mask is all ones
    lay, total = layout(W64)
    assert total == 64
    full = "P %s 31 7 127 255 65535 %d" % (rng(W64), 2**25 - 1)
    assert prog([full])[0].split()[0] == str(2**64 - 1)


def test_cutoff_clamps_at_the_field_maximum(prog):
    cases = []
    for mask in (0, 1, 31, 4095, 65535):
        for base in (INT32_MIN, -30000, 0, 9000, INT32_MAX - mask, INT32_MAX):
            for cutoff in (INT32_MIN, base - 1, base, base + 1,
                           base + mask - 1, base + mask, base + mask + 1,
                           0, INT32_MAX):
                if INT32_MIN <= cutoff <= INT32_MAX:
                    cases.append((cutoff, base, mask))
    got = prog(["C %d %d %d" % c for c in cases])
    for (cutoff, base, mask), ans in zip(cases, got):
        d = cutoff - base
        assert int(ans) == (-1 if d < 0 else min(d, mask)), (cutoff, base,
                                                              mask)


def test_grid_carries_over(prog):
    tpch = 10_000_000 * 100 * 108
    worst = (2**32 - 1) * 100 * 355
    # SF100 at TPC-H prices keeps the default 2048 blocks; the 200,000-row
    # worst-case table of the carry test (59 bits wide, 8 B tier) still
    # needs two blocks under a forced grid of 1
    assert prog(["G 600000000 0 %d" % tpch, "G 200000 1 %d" % worst,
                 "G 1024 0 %d" % worst]) == ["2048", "2", "1"]


def test_fold_fits_its_dwords(prog):
    """count below d_shift and sum(disc) above it share the low dword,
    sum(qty) has the high one; a replica takes the rows of 8 lanes"""
    cases = []
    for n, grid in ((1024, 1), (1027, 1), (200_000, 2), (6_000_000, 2048),
                    (600_000_000, 2048), (600_000_000, 1),
                    (6_000_000_000, 2048), (2**36 + 1, 2048)):
        for qmax in (0, 1, 5100, 65535):
            for dmax in (0, 1, 10, 100):
                cases.append((n, grid, qmax, dmax))
    got = prog(["F %d %d %d %d" % c for c in cases])
    seen = set()
    for (n, grid, qmax, dmax), line in zip(cases, got):
        rows, on, d_shift = (int(x) for x in line.split())
        quads = -(-n // 4)
        iters = -(-quads // (grid * 256))
        assert rows == iters * 8 * 4 + 3
        cb = rows.bit_length()
        fits = cb + (rows * dmax).bit_length() <= 32 and \
            (rows * qmax).bit_length() <= 32
        assert on == int(fits), (n, grid, qmax, dmax)
        seen.add(fits)
        if on:
            assert d_shift == cb and 1 <= d_shift <= 31
            # the worst replica's word: no part reaches its neighbour
            assert rows < 2**d_shift
            assert rows + ((rows * dmax) << d_shift) < 2**32
            assert rows * qmax < 2**32
    assert seen == {True, False}
    # SF100 at TPC-H ranges folds: 9187 rows per replica, 14 + 17 bits
    assert prog(["F 600000000 2048 5100 10"]) == ["9187 1 14"]
    # the GPU test's 200,003 rows of disc 0..100 under a forced grid of 1 do
    # not (6275 rows per replica, 13 + 20 bits) and keep six adds; on the
    # default grid they fold
    assert prog(["F 200003 1 65535 100", "F 200003 196 65535 100"]) == \
        ["6275 0 0", "35 1 6"]
