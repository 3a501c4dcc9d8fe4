"""Exact reference for compiled plans with ORDER BY / LIMIT
(engine_abi.h gg_plan_order, gg_plan_desc.limit).

The groups come from plan_outer_ref.eval_plan, unmodified; this module only
orders them, in Python with big ints, under the rules the header states:

  * order_by entries in turn, ("agg", a, dir[, nulls]) comparing aggregate
    a's value (COUNT / SUM: the exact int; MIN / MAX: the int, None = NULL)
    and ("key", g, dir[, nulls]) comparing group key g (NULL_KEY = NULL);
  * a NULL is placed by the entry's NULL placement whatever the direction;
    omitted, it is PostgreSQL's default: NULLS LAST for "asc", NULLS FIRST
    for "desc" (what the binding fills in);
  * ties are broken by (key0, key1) ascending as raw integers, NULL_KEY
    being the smallest, so the order is total and the result unique;
  * limit > 0 keeps the first `limit` groups, limit == 0 all of them.

An AVG aggregate cannot be an order key (the engine refuses it).
"""
from plan_outer_ref import NULL_KEY, eval_plan  # noqa: F401


def nulls_first(ent):
    """the NULL placement of an order_by entry, defaults filled in"""
    if len(ent) > 3:
        return {"nulls_first": True, "nulls_last": False}[ent[3]]
    return ent[2] == "desc"


def sort_key(order_by):
    """key function over (key0, key1, vals) groups"""
    def key(g):
        out = []
        for ent in order_by:
            what, index, direction = ent[:3]
            if what == "key":
                v = g[index]
                v = None if v == NULL_KEY else v
            else:
                v = g[2][index]
                assert not isinstance(v, tuple), "AVG as an order key"
            nf = nulls_first(ent)
            if v is None:
                out.append((0 if nf else 1, 0))
            else:
                out.append((1 if nf else 0, -v if direction == "desc" else v))
        out.append((g[0], g[1]))
        return tuple(out)
    return key


def order_groups(groups, order_by=(), limit=0):
    """`groups` ordered by order_by and cut to `limit` (0 = all)"""
    out = sorted(groups, key=sort_key(order_by))
    return out[:limit] if limit > 0 else out


def eval_ordered(n, data, nulls, preds, joins, group_cols, aggs,
                 order_by=(), limit=0):
    return order_groups(eval_plan(n, data, nulls, preds, joins, group_cols,
                                  aggs), order_by, limit)
