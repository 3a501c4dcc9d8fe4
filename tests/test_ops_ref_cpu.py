"""tests/ops_ref.py on its own, without a GPU: the collision builders do
what they claim under the oracle's hash functions, and the references are
pinned on hand-written cases, so that tests/test_gpu_ops_edges.py compares
the engine with something that is itself checked."""
import numpy as np
import pytest

import ops_ref as R
import pyoracle


def _h8(k):
    return pyoracle.lib().gg_oracle_hashint8(int(k))


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("nslots,slot", [(4096, 4095), (8192, 8191),
                                         (65536, 65535), (1024, 0)])
def test_colliding_keys_one_hash(nslots, slot, negative):
    keys = R.colliding_keys(2000, nslots, slot, negative=negative)
    assert keys.dtype == np.int64 and len(set(keys.tolist())) == 2000
    assert ((keys < 0) == negative).all()
    hashes = {_h8(k) for k in keys}
    assert len(hashes) == 1                     # the full 32-bit hash
    h = hashes.pop()
    assert h & (nslots - 1) == slot
    for shift in range(20, 32):                 # one spill partition each
        assert {_h8(k) >> shift for k in keys} == {h >> shift}


def test_colliding_keys_prefix_property():
    """A longer family extends a shorter one: what the join test relies on
    when it takes non-members from larger j."""
    a = R.colliding_keys(100, 8192, 8191)
    b = R.colliding_keys(300, 8192, 8191)
    assert np.array_equal(a, b[:100])
    assert 0 not in b.tolist() and R.I64_MIN not in b.tolist()


def test_colliding_strings():
    ss = R.colliding_strings(64, 256, 255)
    assert len(set(ss)) == 64 and all(1 <= len(s) <= 3 for s in ss)
    ha = pyoracle.lib().gg_oracle_hash_any
    assert all(ha(s, len(s)) & 255 == 255 for s in ss)


def test_sort_ref_partial_key_bytes():
    keys = np.array([0x201, 0x100, 0x202, 0x101], np.uint64)
    gk, gp = R.sort_ref(keys, np.arange(4, dtype=np.uint64), 1, False)
    assert gk.tolist() == [0x100, 0x201, 0x101, 0x202]
    assert gp.tolist() == [1, 0, 3, 2]
    gk, gp = R.sort_ref(keys, None, 1, False)
    assert gp is None


def test_sort_ref_descending_two_bytes_upper_nonzero():
    # sorted bytes: 0x0001, 0xFFFF, 0x0001, 0x8000; the upper bytes differ
    # and would reverse the order if they took part
    keys = np.array([0xAA00000000000001, 0x010000000000FFFF,
                     0x0000000000000001, 0xFF00000000008000], np.uint64)
    gk, gp = R.sort_ref(keys, np.arange(4, dtype=np.uint64), 2, True)
    assert gp.tolist() == [1, 3, 0, 2]          # ties keep input order
    assert gk.tolist() == [int(keys[i]) for i in (1, 3, 0, 2)]


def test_sort_ref_full_width_bit63():
    keys = np.array([1 << 63, 0, (1 << 64) - 1, 5], np.uint64)
    assert R.sort_ref(keys, None, 8, False)[0].tolist() == \
        [0, 5, 1 << 63, (1 << 64) - 1]
    assert R.sort_ref(keys, None, 8, True)[0].tolist() == \
        [(1 << 64) - 1, 1 << 63, 5, 0]


def test_groupby_ref_wrapping_sum():
    big = 1 << 62
    k, s, c = R.groupby_ref([7, 7, 7, -3], [big, big, 5, -big])
    assert k.tolist() == [-3, 7]
    # 2^63 + 5 wraps to INT64_MIN + 5
    assert s.tolist() == [-big, R.I64_MIN + 5] and c.tolist() == [1, 3]
    k, s, c = R.groupby_ref([1, 1, 1], [-big, -big, -big])
    assert s.tolist() == [big]                  # -3 * 2^62 mod 2^64


def test_groupby_ref_nulls():
    k, s, c = R.groupby_ref([5, 9, 5, 9, 2], [10, 20, 30, 40, 50],
                            key_nulls=[0, 1, 0, 1, 0],
                            val_nulls=[0, 0, 1, 0, 1])
    assert k.tolist() == [R.NULL_KEY, 2, 5]     # NULL group sorts first
    assert s.tolist() == [60, 0, 10]
    assert c.tolist() == [2, 0, 1]              # group 2 exists, count 0


def test_groupby_bincount_ref_matches_groupby_ref():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 50, 3000)
    vals = rng.integers(-100, 101, 3000)
    a = R.groupby_ref(keys, vals)
    b = R.groupby_bincount_ref(keys, vals, 64)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_join_ref():
    idx, val = R.join_ref([5, -1, R.I64_MIN], [50, 10, 99],
                          [7, -1, 5, 5, 0, R.I64_MIN])
    assert idx.tolist() == [1, 2, 3, 5] and val.tolist() == [10, 50, 50, 99]
    idx, val = R.join_ref([], [], [1, 2])
    assert len(idx) == 0 and idx.dtype == np.int64
    with pytest.raises(AssertionError):
        R.join_ref([1, 1], [2, 3], [1])


def test_dict_ref_orders_bytewise_unsigned():
    codes, d = R.dict_ref([b"ABC", b"AB", b"\x80", b"\x7f", b"", b"AB"])
    assert d == [b"", b"AB", b"ABC", b"\x7f", b"\x80"]
    assert codes.tolist() == [2, 1, 4, 3, 0, 1]
    codes, d = R.dict_ref([b"x", b"", b"x"], nulls=[0, 1, 0])
    assert d == [b"x"] and codes.tolist() == [0, -1, 0]
    codes, d = R.dict_ref([], None)
    assert d == [] and len(codes) == 0
