"""greengage_amd — MI355X-native columnar query-operator engine.

Python face of the C-ABI engine library (libgreengage_engine.so, built
in-tree from csrc/ by `make -C greengage_amd/csrc` or
__graft_entry__.build()).  The compute path is the HIP/CDNA4 engine —
there is NO CPU fallback: on a machine with a GPU, a missing or
unloadable engine library raises immediately.
"""
from .engine import (  # noqa: F401
    AGG_COUNT_DISTINCT,
    ATOM_EQ,
    ATOM_IS_NULL,
    ATOM_LE,
    ATOM_LT,
    ATOM_NE,
    ATOM_NOT_NULL,
    ATOM_NOT_RANGE,
    ATOM_RANGE,
    Engine,
    EngineError,
    HAVING_IS_NULL,
    HAVING_NEG_INF,
    HAVING_NOT_NULL,
    HAVING_NOT_RANGE,
    HAVING_POS_INF,
    HAVING_RANGE,
    JOIN_ANTI,
    JOIN_INNER,
    JOIN_LEFT,
    JOIN_SEMI,
    PGDate,
    PLAN_MAX_ATOMS,
    PLAN_MAX_CLAUSES,
    PLAN_MAX_FILTERS,
    PLAN_MAX_FILTER_PREDS,
    PLAN_MAX_GROUP_COLS,
    PLAN_MAX_HAVING_ATOMS,
    PLAN_MAX_HAVING_CLAUSES,
    PLAN_MAX_HAVING_TOTAL,
    PLAN_MAX_LIMIT,
    PLAN_MAX_ORDER,
    PLAN_MAX_WHERE_ATOMS,
    build_plan_desc,
    build_plan_groups,
    build_plan_having,
    build_plan_where,
    pgdate,
    plan_group_bits,
    plan_group_bits_n,
    plan_topk_tile,
)

__version__ = "0.1.0"
