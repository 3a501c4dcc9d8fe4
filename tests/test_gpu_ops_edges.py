"""Edge-case parity of the standalone operators behind the C ABI (radix
sort, hash group-by plain / NULL-aware / spill, spill hash join, text
dictionary) with the plain references of tests/ops_ref.py.

Every comparison is exact: all values are integers or bytes.  Each shape is
the smallest that reaches its code path; the comment beside it names the
path.  Constants of the code under test that the shapes are derived from:

  radix sort      RS_TILE = 4096 keys per block, 256 threads
  hash tables     nslots = max(1024, next power of two >= 2 * rows)
  group-by        pinned chunked upload above 2^22 rows, 2^24-row chunks
  spill tiers     budget floor 1 MiB; staging chunk = budget / 64 rows
                  (16384 at the floor); group-by spills when 56 * n exceeds
                  the budget, P = pow2_ceil(56 * n / budget + 1); join:
                  need = 48 * nb + 32 * np, same P rule; above 1024
                  partitions the partition kernels change form
  text dict       nslots = max(1024, next power of two >= 4 * max_dict)
"""
import ctypes

import numpy as np
import pytest

import ops_ref as R

pytestmark = pytest.mark.gpu

GG_EINVAL = 1
MIN_BUDGET = 1 << 20
I64 = ctypes.c_int64
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def eng():
    from greengage_amd import Engine
    e = Engine(device=0, n_segments=1, segment_id=0)
    yield e
    e.shutdown()


def _lib():
    from greengage_amd.engine import lib
    return lib()


def _p(a):
    return a.ctypes.data_as(VP)


def _raises_einval(fn, *args, match=None, **kw):
    from greengage_amd.engine import EngineError
    with pytest.raises(EngineError) as ei:
        fn(*args, **kw)
    msg = str(ei.value)
    assert "status %d:" % GG_EINVAL in msg, msg
    if match is not None:
        assert match in msg, msg


def _eq3(got, exp, what=""):
    for g, x, name in zip(got, exp, ("keys", "sums", "counts")):
        assert np.array_equal(g, x), (what, name)


# ======================================================================
# radix sort
# ======================================================================

SORT_N = (1, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)


def _upper_nonzero(keys, key_bytes):
    """Force every byte above the sorted ones to be non-zero."""
    if key_bytes == 8:
        return keys
    mask = (1 << (8 * key_bytes)) - 1
    return keys | np.uint64(0x0101010101010101 & ~mask)


def _check_sort(eng, keys, key_bytes, descending, what):
    n = len(keys)
    pay = np.arange(n, dtype=np.uint64)
    ek, ep = R.sort_ref(keys, pay, key_bytes, descending)
    gk, gp = eng.radix_sort(keys.copy(), pay.copy(), key_bytes=key_bytes,
                            descending=descending)
    assert np.array_equal(gk, ek), what
    assert np.array_equal(gp, ep), what          # stability + pairing


@pytest.mark.parametrize("n", SORT_N)
def test_sort_full_range_all_widths(eng, n):
    """Keys over the whole uint64 range (bit 63 included), every key_bytes,
    both directions, payload arange(n).  Odd key_bytes end in the second
    ping-pong buffer; n around 256 and 4096 are the thread and tile edges;
    12289 = 3 tiles + 1."""
    rng = np.random.default_rng(1000 + n)
    base = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    for kb in range(1, 9):
        keys = _upper_nonzero(base, kb)
        for desc in (False, True):
            _check_sort(eng, keys, kb, desc, (n, kb, desc))


def _structured(kind, kb, rng, n=12289):
    """n keys whose sorted bytes (`low`) follow `kind`, under random
    non-zero bytes above them."""
    mask = (1 << (8 * kb)) - 1
    full = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    upper = _upper_nonzero(full & np.uint64(~mask & R._M64), kb)
    low = rng.integers(0, mask + 1, size=n, dtype=np.uint64)
    if kind == "all_equal":                       # a whole tile on one digit
        low[:] = low[0]
    elif kind == "sorted":
        low.sort()
    elif kind == "reverse":
        low[::-1].sort()
    elif kind == "two_values":
        low = np.where(rng.integers(0, 2, n) == 1, low[0], low[1])
    elif kind == "bytes_00_ff":                   # digits 0 and 255 only
        bits = rng.integers(0, 1 << kb, size=n)
        low = np.zeros(n, np.uint64)
        for b in range(kb):
            low |= np.where((bits >> b) & 1, np.uint64(0xFF << (8 * b)),
                            np.uint64(0))
    elif kind == "ties_1000":
        low = rng.choice(low[:1000], n)
    else:
        raise AssertionError(kind)
    low = low.astype(np.uint64)
    return upper | low if kb < 8 else low


@pytest.mark.parametrize("kind", ["all_equal", "sorted", "reverse",
                                  "two_values", "bytes_00_ff", "ties_1000"])
def test_sort_structured(eng, kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    for kb in (1, 3, 8):
        keys = _structured(kind, kb, rng)
        for desc in (False, True):
            _check_sort(eng, keys, kb, desc, (kind, kb, desc))


@pytest.mark.parametrize("n", [0, 1, 4097])
def test_sort_without_payload(eng, n):
    rng = np.random.default_rng(2000 + n)
    keys = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    for kb, desc in ((8, False), (8, True), (3, True)):
        k = _upper_nonzero(keys, kb)
        gk, gp = eng.radix_sort(k.copy(), key_bytes=kb, descending=desc)
        assert gp is None
        assert np.array_equal(gk, R.sort_ref(k, None, kb, desc)[0]), (kb, desc)


def test_sort_rejects_bad_arguments(eng):
    L = _lib()
    one = np.array([5], np.uint64)
    f = L.gg_engine_radix_sort_u64
    assert f(_p(one), None, 1, 0, 0) == GG_EINVAL
    assert f(_p(one), None, 1, 9, 0) == GG_EINVAL
    # n = 2^32 is past the 32-bit offsets: must return before touching the
    # (one-element) buffer
    assert f(_p(one), None, 1 << 32, 8, 0) == GG_EINVAL
    assert f(_p(one), None, -1, 8, 0) == GG_EINVAL
    assert f(None, None, 1, 8, 0) == GG_EINVAL
    assert one.tolist() == [5]
    keys = np.array([3, 1 << 63, 2, 0], np.uint64)
    gk, gp = eng.radix_sort(keys.copy(), np.arange(4, dtype=np.uint64))
    assert gk.tolist() == [0, 2, 3, 1 << 63] and gp.tolist() == [3, 2, 0, 1]


# ======================================================================
# in-memory group-by
# ======================================================================

EXTREME = [R.I64_MAX, R.I64_MAX - 1, -1, 0, 1, R.I64_MIN + 2]


def _wrapping_vals(rng, n):
    """Values near +-2^62: three of a sign already wrap."""
    mag = (1 << 62) - rng.integers(0, 1000, n)
    return np.where(rng.integers(0, 2, n) == 1, mag, -mag).astype(np.int64)


def _extreme_keys(rng, n, extreme):
    pool = np.array(list(extreme) + rng.integers(
        R.I64_MIN + 2, R.I64_MAX, 10, endpoint=True).tolist(), np.int64)
    keys = pool[rng.integers(0, len(pool), n)]
    m = min(n, len(pool))
    keys[:m] = pool[:m]                          # each extreme key present
    return keys


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 4097])
def test_groupby_extreme_keys_wrapping_sums(eng, n):
    rng = np.random.default_rng(3000 + n)
    vals = _wrapping_vals(rng, n)
    keys = _extreme_keys(rng, n, EXTREME + [R.I64_MIN + 1])
    _eq3(eng.hash_groupby(keys, vals), R.groupby_ref(keys, vals), "plain")
    keys = _extreme_keys(rng, n, EXTREME)
    _eq3(eng.hash_groupby_n(keys, None, vals, None),
         R.groupby_ref(keys, vals), "n, no nulls")
    kn = (rng.random(n) < 0.2).astype(np.uint8)
    vn = (rng.random(n) < 0.3).astype(np.uint8)
    _eq3(eng.hash_groupby_n(keys, kn, vals, vn),
         R.groupby_ref(keys, vals, kn, vn), "n, nulls")


@pytest.mark.parametrize("negative", [False, True])
def test_groupby_chain_wraps_past_last_slot(eng, negative):
    """2000 distinct keys of ONE hash value, one row each: n = 2000 gives
    nslots = 4096, the chain starts on slot 4095 and wraps to slot 0."""
    rng = np.random.default_rng(3100 + negative)
    keys = rng.permutation(R.colliding_keys(2000, 4096, 4095, negative))
    vals = _wrapping_vals(rng, 2000)
    exp = R.groupby_ref(keys, vals)
    assert len(exp[0]) == 2000
    _eq3(eng.hash_groupby(keys, vals), exp, "plain")
    _eq3(eng.hash_groupby_n(keys, None, vals, None), exp, "n")


def test_groupby_chain_with_duplicates(eng):
    """The same chain with 8 rows per key: n = 16000, nslots = 32768, chain
    from slot 32767; find and claim race on every slot of the chain."""
    rng = np.random.default_rng(3200)
    keys = rng.permutation(np.repeat(R.colliding_keys(2000, 32768, 32767),
                                     8))
    vals = _wrapping_vals(rng, len(keys))
    exp = R.groupby_ref(keys, vals)
    assert len(exp[0]) == 2000 and (exp[2] == 8).all()
    _eq3(eng.hash_groupby(keys, vals), exp, "plain")
    _eq3(eng.hash_groupby_n(keys, None, vals, None), exp, "n")


def test_groupby_one_hot_slot(eng):
    rng = np.random.default_rng(3300)
    n = 100_000
    keys = np.full(n, -7, np.int64)
    vals = rng.integers(R.I64_MIN, R.I64_MAX, n, endpoint=True)
    exp = R.groupby_ref(keys, vals)
    _eq3(eng.hash_groupby(keys, vals), exp, "plain")
    vn = (rng.random(n) < 0.5).astype(np.uint8)
    _eq3(eng.hash_groupby_n(keys, None, vals, vn),
         R.groupby_ref(keys, vals, None, vn), "n")


def test_groupby_n_null_shapes(eng):
    rng = np.random.default_rng(3400)
    n = 4097
    keys = rng.integers(-20, 20, n)
    vals = _wrapping_vals(rng, n)
    ones, zeros = np.ones(n, np.uint8), np.zeros(n, np.uint8)
    some = (rng.random(n) < 0.4).astype(np.uint8)
    for what, kn, vn in (("all keys NULL", ones, None),
                         ("all keys NULL, some vals", ones, some),
                         ("all vals NULL", None, ones),     # groups, count 0
                         ("all NULL", ones, ones),
                         ("val_nulls only", None, some),
                         ("key_nulls only", some, None),
                         ("flags given, none set", zeros, zeros)):
        exp = R.groupby_ref(keys, vals, kn, vn)
        _eq3(eng.hash_groupby_n(keys, kn, vals, vn), exp, what)
    exp = R.groupby_ref(keys, vals, None, ones)
    assert (exp[2] == 0).all() and (exp[1] == 0).all() and len(exp[0]) == 40


def test_groupby_cap_too_small(eng):
    L = _lib()
    keys = np.arange(10, dtype=np.int64)
    vals = np.ones(10, np.int64)
    ok, os_, oc = (np.full(10, -5, np.int64) for _ in range(3))
    ng = I64(-1)
    rc = L.gg_engine_hash_groupby_i64(_p(keys), _p(vals), 10, _p(ok), _p(os_),
                                      _p(oc), 5, ctypes.byref(ng))
    assert rc == GG_EINVAL and ng.value == 0
    _eq3(eng.hash_groupby(keys, vals), R.groupby_ref(keys, vals))


def _big_groupby_case(n, seed):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 100_000, n)
    vals = rng.integers(-100, 100, n, endpoint=True)
    return keys, vals, R.groupby_bincount_ref(keys, vals, 100_000)


def test_groupby_pinned_upload_one_chunk(eng):
    """n = 2^22 + 4097: the first n on the pinned, chunked upload path."""
    keys, vals, exp = _big_groupby_case((1 << 22) + 4097, 3500)
    _eq3(eng.hash_groupby(keys, vals), exp)


def test_groupby_pinned_upload_three_chunks(eng):
    """n = 2 * 2^24 + 2^17 + 5: the third chunk reuses the first pinned
    buffer behind its upload event, and its last 2^17-row copy block is
    partial.  The smallest n that reaches the reuse."""
    keys, vals, exp = _big_groupby_case(2 * (1 << 24) + (1 << 17) + 5, 3600)
    _eq3(eng.hash_groupby(keys, vals), exp)


# ======================================================================
# spill group-by
# ======================================================================

def _check_spill_groupby(eng, keys, vals, nparts_exp, what):
    exp = R.groupby_ref(keys, vals)
    k, s, c, nparts = eng.hash_groupby_spill(keys, vals, MIN_BUDGET)
    assert nparts == nparts_exp, (what, nparts)
    _eq3((k, s, c), exp, what + " spill vs ref")
    _eq3(eng.hash_groupby(keys, vals), exp, what + " in-memory vs ref")


def test_spill_groupby_small(eng):
    """n = 40000 under the budget floor: P = 4, three staging chunks (the
    third reuses a staging buffer)."""
    rng = np.random.default_rng(4000)
    n = 40_000
    vals = _wrapping_vals(rng, n)
    keys = rng.integers(R.I64_MIN + 1, R.I64_MAX, n, endpoint=True)
    keys[n // 2:] = rng.integers(-300, 300, n - n // 2)
    _check_spill_groupby(eng, keys, vals, 4, "random")
    # one key: a single non-empty partition, the others skipped
    _check_spill_groupby(eng, np.full(n, 12345, np.int64), vals, 4, "one key")
    keys = _extreme_keys(rng, n, EXTREME + [R.I64_MIN + 1])
    _check_spill_groupby(eng, keys, vals, 4, "extreme")


def test_spill_groupby_chain_in_reload_table(eng):
    """2048 keys of one hash x 16 rows = 32768 rows: P = 2, all rows in one
    partition, so the reload table has 65536 slots and the chain starts on
    its last one."""
    rng = np.random.default_rng(4100)
    keys = rng.permutation(np.repeat(R.colliding_keys(2048, 65536, 65535),
                                     16))
    vals = _wrapping_vals(rng, len(keys))
    _check_spill_groupby(eng, keys, vals, 2, "chain")


def test_spill_groupby_budget_floor(eng):
    keys = np.arange(100, dtype=np.int64)
    _raises_einval(eng.hash_groupby_spill, keys, keys, MIN_BUDGET - 1)
    k, s, c, nparts = eng.hash_groupby_spill(keys, keys, MIN_BUDGET)
    assert nparts == 1
    _eq3((k, s, c), R.groupby_ref(keys, keys))


def test_spill_groupby_2048_partitions(eng):
    """n = 19.2M under the budget floor: P = 2048, past the 1024 partitions
    the LDS-staged count and scatter kernels cover, so the direct-atomic
    forms run.  (19 173 962 rows is the exact threshold.)"""
    keys, vals, exp = _big_groupby_case(19_200_000, 4200)
    k, s, c, nparts = eng.hash_groupby_spill(keys, vals, MIN_BUDGET)
    assert nparts == 2048
    _eq3((k, s, c), exp)


# ======================================================================
# spill join
# ======================================================================

def _join(build_keys, build_vals, probe_keys, budget):
    """gg_engine_hash_join_i64_spill through lib(), returning (status,
    probe_idx, vals, nparts) with the matches in probe_idx order.  An empty
    side is passed as a one-element buffer with n = 0, so that the call
    does not depend on what pointer numpy gives an empty array."""
    def buf(a):
        a = np.ascontiguousarray(a, np.int64)
        return (a if len(a) else np.zeros(1, np.int64)), len(a)
    bk, nb = buf(build_keys)
    bv, _ = buf(build_vals)
    pk, npr = buf(probe_keys)
    oi = np.full(npr + 1, -1, np.int64)
    ov = np.full(npr + 1, -1, np.int64)
    nm, nparts = I64(-1), ctypes.c_int32(-1)
    rc = _lib().gg_engine_hash_join_i64_spill(
        _p(bk), _p(bv), nb, _p(pk), npr, budget, _p(oi), _p(ov), npr + 1,
        ctypes.byref(nm), ctypes.byref(nparts))
    if rc != 0:
        return rc, nm.value, None, nparts.value
    i, v = R.sort_matches(oi[:nm.value], ov[:nm.value])
    return rc, i, v, nparts.value


def _check_join(bk, bv, pk, nparts_spilled, what, ref=R.join_ref):
    ei, ev = ref(bk, bv, pk)
    for budget, nparts_exp in ((MIN_BUDGET, nparts_spilled), (1 << 40, 1)):
        rc, gi, gv, nparts = _join(bk, bv, pk, budget)
        assert rc == 0, (what, budget, rc)
        assert nparts == nparts_exp, (what, budget, nparts)
        assert np.array_equal(gi, ei), (what, budget)
        assert np.array_equal(gv, ev), (what, budget)
    return ei


def _build_side(rng, nb):
    """About nb unique keys over the whole int64 range except 0, with
    INT64_MIN, INT64_MAX, -1 and 1 among them, and full-range values."""
    bk = np.unique(np.concatenate([
        rng.integers(R.I64_MIN, R.I64_MAX, nb - 4, endpoint=True),
        np.array([R.I64_MIN, R.I64_MAX, -1, 1], np.int64)]))
    bk = rng.permutation(bk[bk != 0])
    return bk, rng.integers(R.I64_MIN, R.I64_MAX, len(bk), endpoint=True)


def _absent(rng, bk, n):
    a = rng.integers(R.I64_MIN, R.I64_MAX, n, endpoint=True)
    a[np.isin(a, bk) | (a == 0)] = 2       # 2 is not a build key (asserted)
    assert 2 not in set(bk.tolist())
    return a


def test_spill_join_full_range_keys(eng):
    """nb = 20000, np = 100000 under the budget floor: need = 48 nb + 32 np
    = 4.16 MB, P = 4."""
    rng = np.random.default_rng(5000)
    nb, npr = 20_000, 100_000
    bk, bv = _build_side(rng, nb)
    assert 19_990 <= len(bk) <= nb and 0 not in set(bk.tolist())
    half = npr // 2
    pk = rng.permutation(np.concatenate(
        [rng.choice(bk, half),                         # present, duplicated
         np.array([R.I64_MIN, R.I64_MAX, -1] * 3, np.int64),
         _absent(rng, bk, npr - half - 9)]))
    ei = _check_join(bk, bv, pk, 4, "half present")
    assert half + 9 <= len(ei) < npr
    ei = _check_join(bk, bv, _absent(rng, bk, npr), 4, "no match")
    assert len(ei) == 0
    ei = _check_join(bk, bv, rng.choice(bk, npr), 4, "all match")
    assert len(ei) == npr


def test_spill_join_empty_sides(eng):
    rng = np.random.default_rng(5100)
    bk, bv = _build_side(rng, 20_000)
    pk = rng.choice(bk, 100_000)
    none = np.zeros(0, np.int64)
    # P is computed from the sizes alone: 32 * 100000 B and 48 * 20000 B
    assert len(_check_join(none, none, pk, 4, "nb = 0")) == 0
    assert len(_check_join(bk, bv, none, 1, "np = 0")) == 0
    assert len(_check_join(none, none, none, 1, "both empty")) == 0


def test_spill_join_chain_wraps_past_last_slot(eng):
    """Build side = 3000 keys of one hash value: nslots = 8192, the chain
    starts on slot 8191 and wraps.  The probe mixes members with non-members
    of the same hash (the family continued), which walk the whole chain to
    its empty end.  Spilled (P = 2) the family shares one partition."""
    rng = np.random.default_rng(5200)
    fam = R.colliding_keys(6000, 8192, 8191)
    bk = rng.permutation(fam[:3000])
    bv = rng.integers(R.I64_MIN, R.I64_MAX, 3000, endpoint=True)
    pk = np.concatenate([rng.choice(fam, 38_000),
                         rng.integers(1, 1 << 40, 2_000)])
    ei = _check_join(bk, bv, rng.permutation(pk), 2, "chain")
    assert 15_000 < len(ei) < 23_000


def test_spill_join_2048_partitions(eng):
    """nb = 1000, np = 33.56M under the budget floor: P = 2048, the smallest
    shape on which the index-carrying scatter runs in its direct-atomic form
    (k_gb_part_scatter_idx).  About 1 probe row in 1000 has a partner."""
    rng = np.random.default_rng(5300)
    nb, npr = 1000, 33_560_000
    bk = np.unique(rng.integers(1, 1 << 62, nb))
    bv = rng.integers(R.I64_MIN, R.I64_MAX, len(bk), endpoint=True)
    pk = rng.integers(-(1 << 62), 0, npr)            # absent: negative
    at = rng.choice(npr, npr // 1000, replace=False)
    pk[at] = rng.choice(bk, len(at))
    ei, ev = R.join_searchsorted_ref(bk, bv, pk)
    assert np.array_equal(ei, np.sort(at))
    rc, gi, gv, nparts = _join(bk, bv, pk, MIN_BUDGET)
    assert rc == 0 and nparts == 2048
    assert np.array_equal(gi, ei) and np.array_equal(gv, ev)


# ======================================================================
# reserved values: the contract of include/engine_abi.h
# ======================================================================

def _small_groupby_case(seed, n=10_000):
    rng = np.random.default_rng(seed)
    keys = rng.integers(-500, 500, n)
    vals = rng.integers(-10**9, 10**9, n)
    return keys, vals


def test_groupby_rejects_int64_min(eng):
    """One INT64_MIN key among 10000 rows: GG_EINVAL naming INT64_MIN, not
    a group table in which that row's value went to whichever key claimed
    the slot next.  The next call on the same pooled scratch is correct."""
    keys, vals = _small_groupby_case(6000)
    exp = R.groupby_ref(keys, vals)
    bad = keys.copy()
    bad[4321] = R.I64_MIN
    for _ in range(2):
        _raises_einval(eng.hash_groupby, bad, vals, match="INT64_MIN")
        _eq3(eng.hash_groupby(keys, vals), exp)
    # through lib(): *out_ngroups = 0
    out = [np.zeros(len(bad), np.int64) for _ in range(3)]
    ng = I64(-1)
    rc = _lib().gg_engine_hash_groupby_i64(
        _p(bad), _p(vals), len(bad), _p(out[0]), _p(out[1]), _p(out[2]),
        len(bad), ctypes.byref(ng))
    assert rc == GG_EINVAL and ng.value == 0
    # the spill entry point below its spill threshold takes the same path
    _raises_einval(eng.hash_groupby_spill, bad, vals, MIN_BUDGET,
                   match="INT64_MIN")
    _eq3(eng.hash_groupby(keys, vals), exp)


def test_spill_groupby_rejects_int64_min(eng):
    """The partitioned branch (20000 rows is past the 18724-row threshold
    of the budget floor: P = 2)."""
    keys, vals = _small_groupby_case(6100, 20_000)
    exp = R.groupby_ref(keys, vals)
    for at in (0, 19_999):
        bad = keys.copy()
        bad[at] = R.I64_MIN
        _raises_einval(eng.hash_groupby_spill, bad, vals, MIN_BUDGET,
                       match="INT64_MIN")
        k, s, c, nparts = eng.hash_groupby_spill(keys, vals, MIN_BUDGET)
        assert nparts == 2
        _eq3((k, s, c), exp)


def test_groupby_n_rejects_null_key_code(eng):
    """A non-NULL key of GG_PLAN_NULL_KEY would merge into the NULL group."""
    keys, vals = _small_groupby_case(6200, 1000)
    kn = (np.arange(1000) % 7 == 0).astype(np.uint8)
    exp = R.groupby_ref(keys, vals, kn, None)
    bad = keys.copy()
    bad[501] = R.NULL_KEY
    assert not kn[501]
    _raises_einval(eng.hash_groupby_n, bad, kn, vals, None)
    _raises_einval(eng.hash_groupby_n, bad, None, vals, None)
    _eq3(eng.hash_groupby_n(keys, kn, vals, None), exp)
    # under a NULL flag the value is never read as a key
    bad = keys.copy()
    bad[0] = R.NULL_KEY
    assert kn[0]
    _eq3(eng.hash_groupby_n(bad, kn, vals, None), exp)
    bad[0] = R.I64_MIN
    _raises_einval(eng.hash_groupby_n, bad, None, vals, None,
                   match="INT64_MIN")


def _join_case(seed, nb=20_000, npr=100_000):
    rng = np.random.default_rng(seed)
    bk, bv = _build_side(rng, nb)
    pk = np.concatenate([rng.choice(bk, npr // 2),
                         _absent(rng, bk, npr - npr // 2)])
    return bk, bv, rng.permutation(pk)


@pytest.mark.parametrize("budget,nparts", [(1 << 40, 1), (MIN_BUDGET, 4)])
def test_join_rejects_build_key_zero(eng, budget, nparts):
    bk, bv, pk = _join_case(6300)
    ei, ev = R.join_ref(bk, bv, pk)
    bad = bk.copy()
    bad[777] = 0
    rc, nm, _, _ = _join(bad, bv, pk, budget)
    assert rc == GG_EINVAL and nm == 0
    assert b"key 0" in _lib().gg_engine_last_error()
    # also when no probe row shares the partition of key 0
    rc, nm, _, _ = _join(bad, bv, np.zeros(0, np.int64), budget)
    assert rc == GG_EINVAL and nm == 0
    rc, gi, gv, gp = _join(bk, bv, pk, budget)
    assert rc == 0 and gp == nparts
    assert np.array_equal(gi, ei) and np.array_equal(gv, ev)


@pytest.mark.parametrize("budget,nparts", [(1 << 40, 1), (MIN_BUDGET, 4)])
def test_join_rejects_duplicate_build_key(eng, budget, nparts):
    bk, bv, pk = _join_case(6400)
    ei, ev = R.join_ref(bk, bv, pk)
    bad = bk.copy()
    bad[19_000] = bad[3]                      # one pair, far apart
    rc, nm, _, _ = _join(bad, bv, pk, budget)
    assert rc == GG_EINVAL and nm == 0
    assert b"duplicate" in _lib().gg_engine_last_error()
    rc, gi, gv, gp = _join(bk, bv, pk, budget)
    assert rc == 0 and gp == nparts
    assert np.array_equal(gi, ei) and np.array_equal(gv, ev)


def test_join_probe_key_zero_matches_nothing_sparse_table(eng):
    """Ten build keys in a 1024-slot table: probe key 0 finds its home slot
    empty, which reads as 0, and must not be a match."""
    bk = np.arange(1, 11, dtype=np.int64) * 1_000_003
    bv = -bk
    pk = np.array([0, bk[3], 0, 5, bk[9], 0], np.int64)
    rc, gi, gv, _ = _join(bk, bv, pk, 1 << 40)
    assert rc == 0
    assert gi.tolist() == [1, 4] and gv.tolist() == [-bk[3], -bk[9]]
    rc, gi, gv, _ = _join(bk, bv, np.zeros(1000, np.int64), 1 << 40)
    assert rc == 0 and len(gi) == 0
    # spilled (P = 4): every probe key 0 lands in one partition
    pk = np.zeros(100_000, np.int64)
    pk[::1000] = bk[np.arange(100) % 10]
    rc, gi, gv, nparts = _join(bk, bv, pk, MIN_BUDGET)
    assert rc == 0 and nparts == 4
    assert gi.tolist() == list(range(0, 100_000, 1000))
    assert np.array_equal(gv, -pk[::1000])


def test_join_probe_key_zero_matches_nothing_loaded_table(eng):
    """Build side of exactly 2^12 keys, so its table (2^13 slots) is at the
    highest load a table gets, with 200 keys crowded onto the home slot of
    key 0: the probe for 0 walks a long occupied chain before it reaches an
    empty slot, which must still not be a match."""
    import pyoracle
    rng = np.random.default_rng(6500)
    home = pyoracle.lib().gg_oracle_hashint8(0) & 8191
    crowd = R.colliding_keys(200, 8192, home)
    assert 0 not in set(crowd.tolist())
    rest = _build_side(rng, 4200)[0]
    rest = rest[~np.isin(rest, crowd)][:4096 - 200]
    bk = rng.permutation(np.concatenate([crowd, rest]))
    assert len(bk) == 4096 == len(set(bk.tolist()))
    bv = rng.integers(R.I64_MIN, R.I64_MAX, len(bk), endpoint=True)
    pk = rng.permutation(np.concatenate([np.zeros(500, np.int64),
                                         rng.choice(bk, 1500)]))
    ei, ev = R.join_ref(bk, bv, pk)
    assert len(ei) == 1500
    rc, gi, gv, _ = _join(bk, bv, pk, 1 << 40)
    assert rc == 0
    assert np.array_equal(gi, ei) and np.array_equal(gv, ev)


# ======================================================================
# text dictionary
# ======================================================================

def _check_dict(eng, values, nulls=None, max_dict=4096):
    ec, ed = R.dict_ref(values, nulls)
    codes, d = eng.text_dict_encode(values, nulls, max_dict=max_dict)
    assert d == ed
    assert codes.dtype == np.int32 and np.array_equal(codes, ec)
    return codes, d


def test_dict_small_shapes(eng):
    _check_dict(eng, [])                                   # n = 0
    _check_dict(eng, [b"solo"])                            # n = 1
    _check_dict(eng, [b""])
    _check_dict(eng, [b"x"], nulls=[1])
    _check_dict(eng, [b"BUILDING", b"MACHINERY", b"AUTOMOBILE",
                      b"BUILDING", b"", b"HOUSEHOLD"], nulls=[0, 0, 0, 0, 1,
                                                              0])
    codes, d = _check_dict(eng, [b"a", b"", b"c"] * 50, nulls=[1] * 150)
    assert d == [] and (codes == -1).all()                 # all NULL
    codes, d = _check_dict(eng, [b""] * 300)               # empty strings
    assert d == [b""] and (codes == 0).all()
    _check_dict(eng, [b"", b"b", b"", b"a", b"\x00", b""] * 40)
    # NULL rows whose bytes look like live values
    _check_dict(eng, [b"a", b"b", b"a", b"b"], nulls=[0, 1, 1, 0])


def test_dict_order_is_bytewise_unsigned(eng):
    codes, d = _check_dict(eng, [b"ABC", b"A", b"AB", b"ABC", b"A", b"B"])
    assert d == [b"A", b"AB", b"ABC", b"B"]                # prefix chain
    edge = [bytes([c]) for c in (0x00, 0x7F, 0x80, 0xFF)]
    vals = edge + [c + b"mid" for c in edge] + [b"mid" + c for c in edge] \
        + [b"mid", b"mi", b"\x00\x00", b"\xff\xff", b"\x7f\x80", b"\x80\x7f"]
    rng = np.random.default_rng(7000)
    vals = [vals[i] for i in rng.integers(0, len(vals), 500)] + vals
    codes, d = _check_dict(eng, vals)
    assert d.index(b"\x7f") < d.index(b"\x80") < d.index(b"\xff")
    assert d.index(b"mid") < d.index(b"mid\x00") < d.index(b"mid\xff")


def test_dict_lengths_around_hash_stride(eng):
    """hash_any consumes 12 bytes per round: lengths 11/12/13 and 24/25
    take the tail switch at 11, 0, 1, 0 and 1 bytes.  Pairs differ in the
    last byte only, and one is a prefix of the next."""
    vals = []
    for ln in (11, 12, 13, 24, 25):
        body = bytes(range(65, 65 + ln - 1))
        vals += [body + b"x", body + b"y", body + b"\x00", body + b"\xff"]
    rng = np.random.default_rng(7100)
    rows = [vals[i] for i in rng.integers(0, len(vals), 2000)]
    codes, d = _check_dict(eng, rows + vals)
    assert len(d) == 20


def test_dict_race_to_claim(eng):
    rng = np.random.default_rng(7200)
    vals = [b"AUTOMOBILE", b"", b"BUILDING"]
    rows = [vals[i] for i in rng.integers(0, 3, 100_000)]
    nulls = (rng.random(100_000) < 0.1).astype(np.uint8)
    _check_dict(eng, rows, nulls)
    _check_dict(eng, rows)


def test_dict_max_dict_boundary(eng):
    rng = np.random.default_rng(7300)
    distinct = [b"v%05d" % i for i in range(1001)]
    rows = [distinct[i] for i in rng.permutation(np.arange(3000) % 1000)]
    codes, d = _check_dict(eng, rows, max_dict=1000)       # exactly full
    assert len(d) == 1000
    _raises_einval(eng.text_dict_encode, rows + [distinct[1000]],
                   max_dict=1000, match="dictionary overflow")
    _check_dict(eng, rows, max_dict=1000)


def test_dict_chain_wraps_past_last_slot(eng):
    """64 distinct strings hashing to the last slot of the table that
    max_dict = 64 gives (4 * 64 = 256 is under the 1024-slot floor, so 1024
    slots, slot 1023): one chain of 64, wrapping to slot 0."""
    ss = R.colliding_strings(64, 1024, 1023)
    rng = np.random.default_rng(7400)
    rows = [ss[i] for i in rng.integers(0, 64, 5000)] + ss
    codes, d = _check_dict(eng, rows, max_dict=64)
    assert len(d) == 64


def test_dict_is_permutation_invariant(eng):
    rng = np.random.default_rng(7500)
    distinct = [bytes(rng.integers(0, 256, rng.integers(0, 30),
                                   dtype=np.uint8)) for _ in range(300)]
    pick = rng.integers(0, len(distinct), 20_000)
    rows = [distinct[i] for i in pick]
    nulls = (rng.random(len(rows)) < 0.05).astype(np.uint8)
    codes, d = _check_dict(eng, rows, nulls)
    perm = rng.permutation(len(rows))
    codes2, d2 = _check_dict(eng, [rows[i] for i in perm], nulls[perm])
    assert d2 == d and np.array_equal(codes2, codes[perm])


def test_dict_overflow_is_an_error_return(eng):
    """max_dict = 4 gives the 1024-slot floor table.  40 distinct values
    fit the table and are refused by the host's count; 1100 distinct values
    fill the table, and the rows left over give up after probing all of it
    (the device's bounded "table full" exit).  Both return GG_EINVAL, and
    the next call works."""
    ok_rows = [b"d", b"a", b"c", b"b", b"a"] * 20
    for ndistinct in (40, 1100):
        distinct = [b"k%04d" % i for i in range(ndistinct)]
        _raises_einval(eng.text_dict_encode, distinct * 3, max_dict=4,
                       match="dictionary overflow")
        _check_dict(eng, ok_rows, max_dict=4)


def test_dict_cap_too_small(eng):
    values = [b"alpha", b"beta", b"gamma", b"beta"]
    pool = np.frombuffer(b"".join(values), np.uint8).copy()
    lens = np.array([len(v) for v in values], np.uint32)
    offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    codes = np.zeros(4, np.int32)
    doffs = np.zeros(17, np.int64)
    nd = ctypes.c_int32(-1)

    def call(dcap):
        dbytes = np.zeros(max(dcap, 1), np.uint8)
        rc = _lib().gg_engine_text_dict_encode(
            _p(pool), _p(offs), _p(lens), None, 4, 16, _p(codes), _p(dbytes),
            dcap, _p(doffs), ctypes.byref(nd))
        return rc, dbytes

    for _ in range(3):                       # error exit frees its buffers
        rc, _b = call(13)                    # 5 + 4 + 5 = 14 bytes needed
        assert rc == GG_EINVAL
        assert b"dict_cap" in _lib().gg_engine_last_error()
    rc, dbytes = call(14)
    assert rc == 0 and nd.value == 3
    assert bytes(dbytes[:14]) == b"alphabetagamma"
    assert doffs[:4].tolist() == [0, 5, 9, 14] and codes.tolist() == [0, 1, 2,
                                                                      1]
