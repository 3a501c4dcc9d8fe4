"""Host arithmetic of the packed Q1 companion, without a GPU: the functions
of greengage_amd/csrc/q1_pack.h compiled into a stand-alone program
(q1_pack_host_main.cpp, its own main, built with the address and
undefined-behaviour sanitizers where the compiler has their runtimes) and
asked about the boundary values of the eligibility rules, the grid floor and
the cutoff conversion.  Expectations are computed here in Python integers.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS, ROWS, MAX_BLOCKS = 256, 4, 2048
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("q1pack") / "q1_pack_host")
    src = os.path.join(HERE, "q1_pack_host_main.cpp")
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


OK = dict(n=10, qmin=0, qmax=65535, pmin=0, pmax=2**32 - 1, dmin=0, dmax=100,
          tmin=0, tmax=255, sdmin=-5, sdmax=65530)
ORDER = ("n", "qmin", "qmax", "pmin", "pmax", "dmin", "dmax", "tmin", "tmax",
         "sdmin", "sdmax")


def test_eligibility_boundaries(prog):
    cases = [({}, 1),
             (dict(n=0), 0), (dict(n=1), 1),
             (dict(qmin=-1), 0), (dict(qmax=65536), 0),
             (dict(pmin=-1), 0), (dict(pmax=2**32), 0),
             (dict(dmin=-1), 0), (dict(dmax=101), 0),
             (dict(tmin=-1), 0), (dict(tmax=256), 0),
             (dict(sdmax=65531), 0),             # span 65536
             (dict(sdmin=INT32_MIN, sdmax=INT32_MAX), 0),
             (dict(sdmin=INT32_MIN, sdmax=INT32_MIN + 65535), 1),
             (dict(sdmin=INT32_MAX - 65535, sdmax=INT32_MAX), 1),
             (dict(qmin=-2**63, qmax=2**63 - 1), 0)]
    lines = []
    for change, _ in cases:
        v = dict(OK, **change)
        lines.append("E " + " ".join(str(v[k]) for k in ORDER))
    assert prog(lines) == [str(e) for _, e in cases]


def test_row_bound(prog):
    cases = [(0, 0), (1, 0), (10_000_000, 8), (2**32 - 1, 255), (2**32 - 1, 0)]
    got = prog(["B %d %d" % c for c in cases])
    assert got == [str(p * 100 * (100 + t)) for p, t in cases]
    assert (2**32 - 1) * 100 * 355 < 2**48


def rows_per_block(n, grid):
    quads = -(-n // ROWS)
    iters = -(-quads // (grid * THREADS))
    return iters * THREADS * ROWS + ROWS - 1


def min_grid(n, bound):
    """smallest grid whose blocks cannot wrap a u64, by direct search"""
    cap = max(1, -(-(-(-n // ROWS)) // THREADS))
    lo, hi = 1, cap
    assert rows_per_block(n, cap) * bound < 2**64
    while lo < hi:                      # rows_per_block falls with the grid
        mid = (lo + hi) // 2
        if rows_per_block(n, mid) * bound < 2**64:
            hi = mid
        else:
            lo = mid + 1
    return lo, cap


def test_grid_floor_and_cap(prog):
    worst = (2**32 - 1) * 100 * 355
    tpch = 10_000_000 * 100 * 108
    cases = []
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099, 200_000, 6_000_000,
              600_000_000, 2**36 + 1):
        for bound in (0, 1, tpch, worst):
            for want in (0, 1, 2, 7, 2048, 2**30):
                cases.append((n, want, bound))
    got = prog(["G %d %d %d" % c for c in cases])
    for (n, want, bound), line in zip(cases, got):
        g, rpb, ok = (int(x) for x in line.split())
        floor, cap = min_grid(n, bound)
        asked = want if want > 0 else min(cap, MAX_BLOCKS)
        assert g == min(cap, max(floor, asked)), (n, want, bound)
        assert rpb == rows_per_block(n, g)
        assert ok == 1 and rpb * bound < 2**64
        # every row is some block's: the grid covers the table
        assert rpb * g >= n
    # the cases of the GPU test: 200,000 worst-case rows need two blocks
    assert min_grid(200_000, worst)[0] == 2
    assert prog(["G 200000 1 %d" % worst])[0].split()[0] == "2"
    # SF100 at TPC-H prices keeps the default 2048 blocks
    assert prog(["G 600000000 0 %d" % tpch])[0].split()[0] == "2048"


def test_cutoff_conversion(prog):
    cases = []
    for base in (INT32_MIN, -30000, 0, 9000, INT32_MAX - 65535, INT32_MAX):
        for cutoff in (INT32_MIN, base - 1, base, base + 1, base + 65534,
                       base + 65535, base + 65536, 0, INT32_MAX):
            if INT32_MIN <= cutoff <= INT32_MAX:
                cases.append((cutoff, base))
    got = prog(["C %d %d" % c for c in cases])
    for (cutoff, base), ans in zip(cases, got):
        d = cutoff - base
        assert int(ans) == (-1 if d < 0 else min(d, 65535)), (cutoff, base)
