/*
 * HAVING over a compiled plan's groups (engine_abi.h gg_plan_having): the
 * resolved qual and THE row test.  The device selection (plan_having.hip) and
 * the host path (plan.cpp) both call plan_having_row, so the two cannot
 * drift; tests/plan_having_host_main.cpp compiles this header alone.
 *
 * Plain C++: builds with any C++17 compiler, with or without HIP.  128-bit
 * values are (signed hi, unsigned lo) pairs throughout, never __int128.
 */
#ifndef GG_PLAN_HAVING_H
#define GG_PLAN_HAVING_H

#include <stdint.h>

#include "../../include/engine_abi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_HAVING_HD __host__ __device__
#else
#define GG_HAVING_HD
#endif

namespace gg
{

/* what the value of an atom's aggregate is made of, in a compacted row
 * (code, naggs x (lo, hi)) */
enum PlanHavingVal
{
	PL_HV_I128 = 0,		/* COUNT / SUM: accumulator `slot`, signed
				 * 128-bit, never NULL */
	PL_HV_MIN = 1,		/* MIN / MAX: order-encoded word in `slot`, */
	PL_HV_MAX = 2		/* non-NULL count in `cnt` (0 = NULL) */
};

struct PlanHavingAtomDev
{
	unsigned long long lo_lo;	/* signed 128-bit lo, inclusive */
	long long lo_hi;
	unsigned long long hi_lo;	/* signed 128-bit hi, exclusive */
	long long hi_hi;
	int8_t kind;		/* gg_plan_havingkind */
	int8_t val;		/* PlanHavingVal */
	int8_t slot;
	int8_t cnt;
};

/* the clauses' atoms back to back, clause c owning natoms[c] of them */
struct PlanHavingDev
{
	PlanHavingAtomDev atoms[GG_PLAN_MAX_HAVING_TOTAL];
	int8_t natoms[GG_PLAN_MAX_HAVING_CLAUSES];
	int nclauses;
};

/* a < b over signed 128-bit (hi, lo) pairs */
GG_HAVING_HD static inline bool
plan_having_lt(long long ah, unsigned long long al, long long bh,
	       unsigned long long bl)
{
	return ah != bh ? ah < bh : al < bl;
}

/* One atom over one compacted row.  The value is read as plan_write_arena
 * decodes it: a MAX word is x ^ MSB, a MIN word its complement, and N = 0
 * makes either SQL NULL. */
GG_HAVING_HD static inline bool
plan_having_atom(const PlanHavingAtomDev &A, const unsigned long long *row)
{
	unsigned long long vl = row[1 + 2 * A.slot];
	long long vh;
	bool null = false;

	if (A.val == PL_HV_I128)
		vh = (long long) row[2 + 2 * A.slot];
	else
	{
		unsigned long long e = A.val == PL_HV_MIN ? ~vl : vl;

		vl = e ^ 0x8000000000000000ull;
		vh = (long long) vl < 0 ? -1 : 0;
		null = row[1 + 2 * A.cnt] == 0;
	}
	if (A.kind == GG_HAVING_IS_NULL)
		return null;
	if (A.kind == GG_HAVING_NOT_NULL)
		return !null;
	/* INT128_MIN below is no test by itself; INT128_MAX above is the
	 * "no upper test" sentinel */
	const bool open_hi = A.hi_hi == INT64_MAX && A.hi_lo == ~0ull;
	const bool in = !plan_having_lt(vh, vl, A.lo_hi, A.lo_lo) &&
		(open_hi || plan_having_lt(vh, vl, A.hi_hi, A.hi_lo));

	return !null && in == (A.kind == GG_HAVING_RANGE);
}

/* true iff the row's group passes the HAVING: every clause has a true atom */
GG_HAVING_HD static inline bool
plan_having_row(const PlanHavingDev &H, const unsigned long long *row)
{
	int at = 0;
	bool all = true;

	for (int c = 0; c < H.nclauses; c++)
	{
		bool any = false;

		for (int q = 0; q < H.natoms[c]; q++)
			any |= plan_having_atom(H.atoms[at + q], row);
		at += H.natoms[c];
		all &= any;
	}
	return all;
}

}				/* namespace gg */

#endif /* GG_PLAN_HAVING_H */
