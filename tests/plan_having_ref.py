"""Exact reference for compiled plans with HAVING (engine_abi.h
gg_plan_having).

The groups come from plan_outer_ref.eval_plan (or any evaluator with its
result form), unmodified; this module only filters them, in Python with big
ints, under the rules the header states:

  * `having` is a list of clauses, ANDed; a clause is one atom or a list of
    atoms, ORed; an atom is the binding's: ("range", a, lo, hi),
    ("not_range", a, lo, hi), ("cmp", a, op, v), ("in", a, [v...]),
    ("is_null", a), ("not_null", a), `a` an index into the group's values;
  * a value is the group's aggregate as execute_plan reports it: an int for
    COUNT / SUM (never NULL), an int or None (NULL) for MIN / MAX; an AVG
    tuple is an assertion error;
  * comparisons over a NULL are not true, is_null is true exactly then;
  * lo is inclusive and hi exclusive; lo == I128_MIN is no lower test and
    hi == I128_MAX no upper test; not_range is the complement of range on
    non-NULL values.

It composes with plan_order_ref.order_groups: filter, then order and limit.
"""
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1

_OPS = {"<": lambda v, x: v < x, "<=": lambda v, x: v <= x,
        "=": lambda v, x: v == x, "<>": lambda v, x: v != x,
        ">": lambda v, x: v > x, ">=": lambda v, x: v >= x}


def in_range(v, lo, hi):
    return (lo == I128_MIN or v >= lo) and (hi == I128_MAX or v < hi)


def atom_true(atom, vals):
    tag, a = atom[0], atom[1]
    v = vals[a]
    assert not isinstance(v, tuple), "AVG in a HAVING"
    if tag == "is_null":
        return v is None
    if tag == "not_null":
        return v is not None
    if v is None:
        return False
    if tag == "range":
        return in_range(v, atom[2], atom[3])
    if tag == "not_range":
        return not in_range(v, atom[2], atom[3])
    if tag == "cmp":
        return _OPS[atom[2]](v, atom[3])
    if tag == "in":
        return any(v == x for x in atom[2])
    raise AssertionError(f"unknown having atom {atom!r}")


def is_atom(c):
    return isinstance(c, tuple) and len(c) > 0 and isinstance(c[0], str)


def passes(having, vals):
    """true iff every clause has a true atom"""
    return all(any(atom_true(t, vals) for t in ([cl] if is_atom(cl) else cl))
               for cl in having)


def filter_groups(groups, having):
    """the (key0, key1, vals) groups that pass `having`, in their order"""
    return [g for g in groups if passes(having, g[2])]
