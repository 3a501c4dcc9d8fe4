/*
 * What the two executors of a compiled plan share on the device: the
 * argument structs, the sentinels and error bits, and the group-table and
 * two-word-accumulator functions.  The interpreted kernel (plan.hip) gets
 * this header through engine_internal.h; plan_rtc.cpp carries its TEXT,
 * behind that of gg_pg_hash.h, at the head of every program it generates
 * (Makefile, plan_dev_src.inc).  ONE definition for both, so the two cannot
 * drift.
 *
 * Three settings compile it: host C++, HIP (hipcc), and hipRTC, where no
 * header can be included.  A generated program therefore starts with
 * #define lines for the GG_PLAN_MAX_* bounds, formatted from the host's own
 * engine_abi.h values, and for PLAN_DEV_TAIL (below).
 */
#ifndef GG_PLAN_DEV_H
#define GG_PLAN_DEV_H

#ifdef __HIPCC_RTC__
typedef long long int64_t;
typedef unsigned long long uint64_t;
typedef unsigned int uint32_t;
typedef int int32_t;
typedef unsigned char uint8_t;
typedef signed char int8_t;
#else
#include <stdint.h>

#include "../../include/engine_abi.h"
#include "../../include/gg_pg_hash.h"
/* How many of the trailing blocks PlanDev carries: 0 = it ends after `pl`,
 * 1 = `gp` follows, 2 = `gp` and `fl`, 3 = `gp`, `fl` and `wh`, 4 = those and
 * `gn`.  The host and plan.hip always see 2.  A generated program is compiled at the lowest level
 * that holds what its plan reads, and launched with exactly that many bytes
 * (plan_rtc.cpp plan_arg_bytes): a plan without a packed group pair, an
 * aggregate filter or WHERE clauses keeps the argument block, and with it
 * the binary, it always had.  Levels 3 and 4 exist in generated programs only
 * (see PlanWhereDev and PlanGroupNDev). */
#define PLAN_DEV_TAIL 2
#endif

namespace gg
{

struct PlanPredDev
{
	const void *col;
	const uint8_t *nulls;
	int width;
	int64_t lo, hi;
};

struct PlanJoinDev
{
	const void *pkey;
	const uint8_t *pnulls;
	int width;
	const unsigned long long *bits;	/* dense membership bitmap, or */
	int64_t dlen;
	const unsigned long long *hkeys;	/* hash semi-set (key^msb, 0=empty) */
	uint64_t hslots;
};

/* dense index map "no build row"; INNER and LEFT build sides stay below
 * it.  It is also what a LEFT join leaves in a row's index when the row
 * has no partner (NULL-extended): the kernels test for it AHEAD of every
 * address computation, NULL-flag loads included, and never load with it */
#define PL_NOROW 0xFFFFFFFFu
/* bits of the plan error word (PlanDev.err) */
#define PL_ERR_FULL 1ull	/* group table full */
#define PL_ERR_BAKE_MISS 2ull	/* baked kernel met an unbaked code */
#define PL_ERR_DUP_KEY 4ull	/* INNER build key not unique, INT64_MIN or
				 * outside the dense map */
/* the sign bit: a join's hash table stores key ^ PL_MSB (0 = empty), and
 * the MIN/MAX words are order-encoded with it (PlanAggDev) */
#define PL_MSB 0x8000000000000000ull
/* an unused group-table key: the INT64_MIN pattern, never a group code */
#define PL_EMPTY 0x8000000000000000ull

/* One device accumulator slot (two u64 words).  kind 0..2 are the
 * descriptor's COUNT(*) / COUNT(factors non-NULL) / SUM; plan.cpp
 * lowers MIN, MAX and AVG onto these plus two order-encoded kinds:
 *   3 = MIN word: ~(x ^ 0x8000000000000000)   } combined by UNSIGNED
 *   4 = MAX word:   x ^ 0x8000000000000000    } max; word 1 unused
 * Zero is the identity of both, so zero-initialised tables and the
 * skip-zero flushes need no special case; the paired count slot tells
 * "no input" from a real INT64_MAX / INT64_MIN. */
struct PlanAggDev
{
	int kind;		/* 0..4, see above */
	int nf;
	const void *col[3];
	const uint8_t *nulls[3];
	int width[3];
	int8_t mod[3];		/* gg_plan_fmod */
};

/* What INNER joins add to a plan, kept in ONE block at the end of
 * PlanDev: every field a plan without an INNER join reads keeps the
 * offset it always had, so those plans' kernels stay the binaries they
 * were (the interpreted kernel reads its descriptor through scalar
 * loads in the row loop and was measurably slower on the Q1 shape when
 * the join and aggregate entries merely grew: DESIGN.md, "Inner joins
 * with payload columns").  Sources: 0 = the driving
 * table, 1+k = the build table of INNER or LEFT join k.  A LEFT join is
 * built and laid out as an INNER one, an ANTI join as a SEMI one; jkind
 * tells the probe what to do with the answer. */
struct PlanPayloadDev
{
	/* INNER / LEFT join j: key -> build-row-index map instead of a membership
	 * set (joins[j].bits stays NULL).  joins[j].dlen > 0: dense,
	 * jidx[j][key], PL_NOROW = absent; else jidx[j][] runs parallel to
	 * joins[j].hkeys[], written only where a key was installed */
	const uint32_t *jidx[GG_PLAN_MAX_JOINS];
	int8_t jkind[GG_PLAN_MAX_JOINS];	/* gg_plan_joinkind */
	int8_t jpsrc[GG_PLAN_MAX_JOINS];	/* source of joins[j].pkey */
	int8_t gsrc[2];				/* source of gcol[g] */
	int8_t asrc[GG_PLAN_MAX_AGGS][3];	/* source of aggs[a].col[f] */
};

/* Packed two-column group code (engine_abi.h gg_plan_desc.group_cols):
 * code = (e0 << shift) | e1, e_g = 0 for NULL, else v - gmin[g] + 1.
 * Set for every ngroup == 2 plan but the (char1, char1) pair, which
 * keeps e0 * 512 + e1; filled at the plan's first execute, when the
 * column ranges are resolved.  Appended after `pl` for the reason given
 * there: no field of today's plans moves. */
struct PlanGroupPackDev
{
	int packed;
	int shift;		/* b1, the width of e1 */
	int64_t gmin[2];
};

/* Aggregate filters (engine_abi.h gg_plan_filter), appended after `gp`
 * under the rule given at PlanPayloadDev: no field an existing plan reads
 * may move, so a plan without a referenced filter keeps its kernels.
 * Filter k keeps its descriptor index; `used` has bit k set iff some
 * accumulator slot references it (only those are evaluated, once per
 * row), afilt[a] is slot a's filter, 0 = none, 1+k = filter k.  A helper
 * count slot carries its aggregate's filter.  The generated kernels read
 * the block in place (P.fl; their PlanDev holds it, and the launch passes
 * its bytes, only when `used` is non-zero: PLAN_DEV_TAIL); the interpreted
 * kernel gets a copy as an argument of its own (plan.hip PlFilters). */
struct PlanFilterDev
{
	PlanPredDev preds[GG_PLAN_MAX_FILTERS][GG_PLAN_MAX_FILTER_PREDS];
	int8_t psrc[GG_PLAN_MAX_FILTERS][GG_PLAN_MAX_FILTER_PREDS];
	int8_t npreds[GG_PLAN_MAX_FILTERS];
	int8_t afilt[GG_PLAN_MAX_AGGS];
	int used;		/* bit k: filter k is referenced */
};

/* General WHERE clauses (engine_abi.h gg_plan_where), lowered: the atoms of
 * one scope, clause after clause; clause c owns natoms[c] consecutive atoms.
 * For scope 0 the first nscan clauses read the driving table alone (scan
 * clauses, evaluated with the scan preds ahead of the joins), the others
 * read some payload column (post-join clauses, evaluated once per row that
 * survived preds and joins, ahead of the aggregate filters and the group
 * code).  A build scope holds scan clauses only.
 *
 * The block is NOT a member of the host's PlanDev.  The rule given at
 * PlanPayloadDev (no field an existing plan reads may move) would allow
 * appending it, but the interpreted kernel already carries PlanDev plus a
 * PlFilters copy in its kernarg segment and a member here would be a third
 * copy past the 4 KiB a launch may pass.  It reaches the interpreted kernel
 * as an argument of its own (plan.hip PlWhere), k_plan_build as the last
 * member of PlanBuildDev, and the generated kernels as the member `wh` that
 * only PLAN_DEV_TAIL 3 declares: plan_rtc_launch lays the block directly
 * behind the host PlanDev's bytes (plan_rtc.cpp PlanDevWhere). */
struct PlanAtomDev
{
	const void *col, *col2;			/* a, b (comparisons only) */
	const uint8_t *nulls, *nulls2;
	int64_t lo, hi;
	int8_t kind;				/* gg_plan_atomkind */
	int8_t src, src2;			/* column sources */
	int8_t width, width2;
};

struct PlanWhereDev
{
	PlanAtomDev atoms[GG_PLAN_MAX_WHERE_ATOMS];
	int8_t natoms[GG_PLAN_MAX_CLAUSES];
	int8_t nclauses;
	int8_t nscan;
};

/* Three or four group columns (engine_abi.h gg_plan_groups), packed into one
 * code of G fields, field 0 most significant:
 *   code = e0 << shift[0] | e1 << shift[1] | ... | e(G-1),
 * e_g as in PlanGroupPackDev, shift[g] = the summed widths of the fields
 * behind field g (shift[G-1] = 0).  PlanKeysN is all a decoder needs
 * (plan_keys.h); n = 0 says "not such a plan", and the code is then read by
 * PlanGroupPackDev / ngroup as ever. */
#define PL_MAX_GCOLS 4		/* GG_PLAN_MAX_GROUP_COLS */

struct PlanKeysN
{
	int n;			/* G: 3 or 4, or 0 */
	int shift[PL_MAX_GCOLS];
	int64_t gmin[PL_MAX_GCOLS];
};

/* What a G >= 3 plan adds to the scan: group columns 2 and 3 (columns 0 and 1
 * stay PlanDev.gcol / gnulls / gwidth / pl.gsrc) and the code's parameters,
 * filled at the plan's first execute.
 *
 * Like PlanWhereDev, and for the same reasons, the block is NOT a member of
 * the host's PlanDev: sizeof(PlanDev) and every offset in it stay what they
 * were, no existing plan's argument block or program changes, and the
 * interpreted kernel's arguments stay inside the 4 KiB a launch may pass.
 * It rides BEHIND `wh`: a generated program of a G >= 3 plan is compiled at
 * PLAN_DEV_TAIL 4, whose PlanDev declares `wh` and then `gn`, and
 * plan_rtc_launch lays PlanWhereDev (all zero for a plan without clauses,
 * which the program then never reads) and this block directly behind the
 * host PlanDev's bytes (plan_rtc.cpp PlanDevGroupN).  The interpreted kernel
 * gets it in the same argument that carries its clauses (plan.hip
 * PlWhereN). */
struct PlanGroupNDev
{
	const void *gcol[PL_MAX_GCOLS - 2];
	const uint8_t *gnulls[PL_MAX_GCOLS - 2];
	int gwidth[PL_MAX_GCOLS - 2];
	int8_t gsrc[PL_MAX_GCOLS - 2];
	PlanKeysN k;
};

struct PlanDev
{
	int64_t n;
	int npreds, njoins, naggs, ngroup;
	PlanPredDev preds[GG_PLAN_MAX_PREDS];
	PlanJoinDev joins[GG_PLAN_MAX_JOINS];
	const void *gcol[2];
	const uint8_t *gnulls[2];
	int gwidth[2];
	unsigned long long *tkeys;	/* nslots; PL_EMPTY = unused */
	unsigned long long *tvals;	/* nslots * naggs * 2 (lo, hi) */
	uint64_t nslots;
	unsigned long long *err;
	PlanAggDev aggs[GG_PLAN_MAX_AGGS];
	PlanPayloadDev pl;
#if PLAN_DEV_TAIL >= 1
	PlanGroupPackDev gp;
#endif
#if PLAN_DEV_TAIL >= 2
	PlanFilterDev fl;
#endif
#if PLAN_DEV_TAIL >= 3
	PlanWhereDev wh;
#endif
#if PLAN_DEV_TAIL >= 4
	PlanGroupNDev gn;
#endif
};

#ifdef __HIPCC__
/* group-table find-or-create (execHHashagg.c:905); -1 = table full */
__device__ static inline int64_t
pl_slot(const PlanDev &P, long long code)
{
	uint64_t pos = (uint64_t) gg_hashint8(code) & (P.nslots - 1);

	for (uint64_t it = 0; it < P.nslots; it++)
	{
		unsigned long long cur = P.tkeys[pos];

		if (cur == (unsigned long long) code)
			return (int64_t) pos;
		if (cur == PL_EMPTY)
		{
			unsigned long long prev =
				atomicCAS(&P.tkeys[pos], PL_EMPTY,
					  (unsigned long long) code);

			if (prev == PL_EMPTY ||
			    prev == (unsigned long long) code)
				return (int64_t) pos;
			continue;
		}
		pos = (pos + 1) & (P.nslots - 1);
	}
	return -1;
}

/* exact two-word add into registers */
__device__ static inline void
pl_add128(unsigned long long &lo, unsigned long long &hi,
	  unsigned long long vlo, unsigned long long vhi)
{
	unsigned long long old = lo;

	lo += vlo;
	hi += vhi + (lo < old);
}

/* ... and into an accumulator w[0..1] in LDS or global memory; the
 * carry comes from the returned old low word */
__device__ static inline void
pl_atomic_add128(unsigned long long *w, unsigned long long vlo,
		 unsigned long long vhi)
{
	unsigned long long old = atomicAdd(w, vlo);

	if (old + vlo < old)
		vhi++;
	if (vhi)
		atomicAdd(w + 1, vhi);
}
#endif				/* __HIPCC__ */

}				/* namespace gg */

#endif /* GG_PLAN_DEV_H */
