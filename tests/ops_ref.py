"""Plain references and input builders for the standalone operators behind
the C ABI: radix sort, hash group-by (plain, NULL-aware, spill), the spill
hash join and the text dictionary.

numpy and Python integers only; nothing here calls the engine.  The two
collision builders use the CPU oracle's hash functions (oracle/), which
tests/test_hash_cpu.py pins against the reference's own hashfunc.c.
"""
import itertools

import numpy as np

I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1
NULL_KEY = I64_MIN + 1          # GG_PLAN_NULL_KEY
_M64 = (1 << 64) - 1


def _wrap64(x):
    """Python int -> the int64 with the same low 64 bits."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


# ---- radix sort ---------------------------------------------------------

def sort_ref(keys, payload, key_bytes, descending):
    """Stable sort of uint64 keys by their low `key_bytes` bytes; bytes above
    do not influence the order.  Descending = ascending on the keys XOR inv,
    inv as in the ABI comment: all ones over the sorted bytes.  Returns
    (keys permuted, payload permuted or None)."""
    keys = np.asarray(keys, np.uint64)
    assert 1 <= key_bytes <= 8
    mask = np.uint64(_M64 if key_bytes == 8 else (1 << (8 * key_bytes)) - 1)
    inv = mask if descending else np.uint64(0)
    order = np.argsort((keys ^ inv) & mask, kind="stable")
    pay = None if payload is None else np.asarray(payload, np.uint64)[order]
    return keys[order], pay


# ---- group-by -----------------------------------------------------------

def groupby_ref(keys, vals, key_nulls=None, val_nulls=None):
    """(keys, sums, counts) sorted by key.  Sums wrap as two's-complement
    int64 (computed mod 2^64 with Python ints); a NULL val is skipped by the
    sum and the count (strict), its key's group still exists; a NULL key is
    reported as GG_PLAN_NULL_KEY."""
    groups = {}
    kn = None if key_nulls is None else np.asarray(key_nulls)
    vn = None if val_nulls is None else np.asarray(val_nulls)
    for i, (k, v) in enumerate(zip(np.asarray(keys, np.int64).tolist(),
                                   np.asarray(vals, np.int64).tolist())):
        if kn is not None and kn[i]:
            k = NULL_KEY
        g = groups.setdefault(k, [0, 0])
        if vn is None or not vn[i]:
            g[0] += v
            g[1] += 1
    ks = sorted(groups)
    return (np.array(ks, np.int64),
            np.array([_wrap64(groups[k][0]) for k in ks], np.int64),
            np.array([groups[k][1] for k in ks], np.int64))


def groupby_bincount_ref(keys, vals, nkeys):
    """The same for large inputs with keys in [0, nkeys) and small values:
    two np.bincount calls.  The weighted sums are float64 and exact while
    every |sum| stays below 2^53 (asserted)."""
    keys = np.asarray(keys, np.int64)
    cnt = np.bincount(keys, minlength=nkeys)
    assert int(np.abs(vals).max()) * int(cnt.max()) < 1 << 53
    sums = np.bincount(keys, weights=vals, minlength=nkeys)
    present = np.nonzero(cnt)[0]
    return (present.astype(np.int64), sums[present].astype(np.int64),
            cnt[present].astype(np.int64))


# ---- join ---------------------------------------------------------------

def join_ref(build_keys, build_vals, probe_keys):
    """(probe_idx, val) for every probe row with a partner, ascending
    probe_idx.  Build keys are taken as unique (asserted)."""
    bk = np.asarray(build_keys, np.int64).tolist()
    table = dict(zip(bk, np.asarray(build_vals, np.int64).tolist()))
    assert len(table) == len(bk), "join_ref: duplicate build keys"
    idx, val = [], []
    for i, k in enumerate(np.asarray(probe_keys, np.int64).tolist()):
        v = table.get(k)
        if v is not None:
            idx.append(i)
            val.append(v)
    return np.array(idx, np.int64), np.array(val, np.int64)


def join_searchsorted_ref(build_keys, build_vals, probe_keys):
    """join_ref for probe sides too large for a Python loop: binary search
    of every probe key in the sorted (unique) build keys."""
    bk = np.asarray(build_keys, np.int64)
    bv = np.asarray(build_vals, np.int64)
    pk = np.asarray(probe_keys, np.int64)
    if len(bk) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(bk, kind="stable")
    sk = bk[order]
    assert (sk[1:] != sk[:-1]).all(), "duplicate build keys"
    at = np.minimum(np.searchsorted(sk, pk), len(sk) - 1)
    idx = np.nonzero(sk[at] == pk)[0]
    return idx.astype(np.int64), bv[order][at[idx]]


def sort_matches(probe_idx, vals):
    """The engine emits matches in no particular order; probe_idx is unique
    per match (unique build keys), so sorting by it is canonical."""
    order = np.argsort(probe_idx, kind="stable")
    return probe_idx[order], vals[order]


# ---- text dictionary ----------------------------------------------------

def dict_ref(values, nulls=None):
    """(codes int32, dictionary): the dictionary is sorted(set(non-NULL
    values)) under Python's bytewise (unsigned) bytes order; codes index it,
    -1 for NULL."""
    live = [v for i, v in enumerate(values)
            if nulls is None or not nulls[i]]
    d = sorted(set(live))
    code = {v: i for i, v in enumerate(d)}
    codes = np.array([-1 if (nulls is not None and nulls[i]) else code[v]
                      for i, v in enumerate(values)], np.int32)
    return codes.reshape(len(values)), d


# ---- collision builders -------------------------------------------------

def _oracle():
    import pyoracle
    return pyoracle.lib()


def colliding_keys(m, nslots, slot, negative=False):
    """m distinct int64 keys with one and the same hashint8 value whose low
    bits, in a table of `nslots` (a power of two), give `slot`.

    hashint8 folds the key's 32-bit halves (lo ^ hi for v >= 0, lo ^ ~hi
    for v < 0) and hashes the fold, so every key with fold c hashes like c:
      non-negative  hi = j,              lo = c ^ j
      negative      hi = 0x80000000 | j, lo = c ^ ~hi      (j = 0, 1, ...)
    c is the first value >= 1 whose hash lands on `slot`."""
    assert nslots & (nslots - 1) == 0 and 0 <= slot < nslots
    h8 = _oracle().gg_oracle_hashint8
    c = 1
    while h8(c) & (nslots - 1) != slot:
        c += 1
    out = []
    for j in range(m):
        if negative:
            hi = 0x80000000 | j
            lo = c ^ (~hi & 0xFFFFFFFF)
        else:
            hi = j
            lo = c ^ j
        out.append(_wrap64((hi << 32) | lo))
    return np.array(out, np.int64)


def colliding_strings(m, nslots, slot):
    """m distinct short byte strings whose hash_any value has low bits `slot`
    in a table of `nslots`: brute force over 1-, 2-, 3-byte strings."""
    assert nslots & (nslots - 1) == 0 and 0 <= slot < nslots
    ha = _oracle().gg_oracle_hash_any
    out = []
    for ln in (1, 2, 3):
        for t in itertools.product(range(256), repeat=ln):
            s = bytes(t)
            if ha(s, ln) & (nslots - 1) == slot:
                out.append(s)
                if len(out) == m:
                    return out
    raise AssertionError("colliding_strings: search space exhausted")
