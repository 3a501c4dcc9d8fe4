/*
 * COUNT(DISTINCT x) over a compiled plan (engine_abi.h gg_plan_aggkind): the
 * regroup that folds the inner plan's groups, one per (group key, value)
 * pair, into the descriptor's groups.  The device kernel (plan_distinct.hip)
 * and the host path (plan.cpp) both fold with plan_regroup_code and
 * plan_regroup_contrib, so the two cannot drift;
 * tests/plan_distinct_host_main.cpp compiles this header alone.
 *
 * Plain C++: builds with any C++17 compiler, with or without HIP.  128-bit
 * values are (lo, hi) word pairs throughout, never __int128.
 */
#ifndef GG_PLAN_DISTINCT_H
#define GG_PLAN_DISTINCT_H

#include <stdint.h>

#include <map>
#include <vector>

#include "plan_keys.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_DISTINCT_HD __host__ __device__
#else
#define GG_DISTINCT_HD
#endif

namespace gg
{

/* What the fold knows of the inner plan: how its group code is laid out
 * (the outer group column first, the distinct column last) and what every
 * accumulator slot of a compacted row (code, naggs x (lo, hi)) holds.  The
 * fold keeps the slot layout: outer rows are read like inner ones. */
struct PlanRegroupDev
{
	PlanGroupPackDev gp;	/* packed, shift, gmin[] of the inner code */
	int ngroup;		/* of the inner plan: the outer one's + 1 */
	int naggs;
	int8_t kind[GG_PLAN_MAX_AGGS];	/* PlanAggDev.kind of every slot */
	unsigned dmask;		/* bit a: slot a is a DISTINCT aggregate's
				 * COUNT(x) */
};

/* The code a plan grouping by the outer column alone would have produced:
 * the raw value or GG_PLAN_NULL_KEY, and 0 for a plan without a group
 * column. */
GG_DISTINCT_HD static inline long long
plan_regroup_code(const PlanRegroupDev &G, long long inner_code)
{
	int64_t k0, k1;

	if (G.ngroup < 2)
		return 0;
	plan_keys_of(G.gp, G.ngroup, inner_code, &k0, &k1);
	return k0;
}

/* What the inner slot a = (lo, hi) adds to the same slot of its outer group;
 * false = nothing.  COUNT / SUM slots add their 128-bit value; the encoded
 * MIN / MAX word combines by unsigned max, 0 being "no input"; a distinct
 * slot holds how many rows carried the pair's value, and the value counts
 * once if any did. */
GG_DISTINCT_HD static inline bool
plan_regroup_contrib(const PlanRegroupDev &G, int a, unsigned long long lo,
		     unsigned long long hi, unsigned long long *vlo,
		     unsigned long long *vhi)
{
	if (G.dmask >> a & 1)
	{
		*vlo = 1;
		*vhi = 0;
		return (lo | hi) != 0;
	}
	if (G.kind[a] >= 3)
	{
		*vlo = lo;
		*vhi = 0;
		return lo != 0;
	}
	*vlo = lo;
	*vhi = hi;
	return (lo | hi) != 0;
}

/* The host's fold: rows_in are compacted inner rows, rows_out the outer
 * ones, ordered by outer code like the output of plan_combine_segments.
 * Every inner row finds or creates its outer group, so a group whose values
 * are all NULL is there with count 0.  No input rows give no output rows,
 * also for a plan without a group column: its one row (code 0, zeros) is the
 * caller's to supply. */
static inline void
plan_regroup_rows(const PlanRegroupDev &G,
		  const std::vector<unsigned long long> &rows_in,
		  std::vector<unsigned long long> *rows_out)
{
	const size_t rowsz = 1 + 2 * (size_t) G.naggs;
	std::map<long long, std::vector<unsigned long long>> merged;

	for (size_t i = 0; i + rowsz <= rows_in.size(); i += rowsz)
	{
		const unsigned long long *row = &rows_in[i];
		std::vector<unsigned long long> &acc =
			merged[plan_regroup_code(G, (long long) row[0])];

		if (acc.empty())
			acc.assign(2 * (size_t) G.naggs, 0);
		for (int a = 0; a < G.naggs; a++)
		{
			unsigned long long vlo, vhi;

			if (!plan_regroup_contrib(G, a, row[1 + 2 * a],
						  row[2 + 2 * a], &vlo, &vhi))
				continue;
			if (G.kind[a] >= 3)	/* never a distinct slot */
			{
				if (vlo > acc[2 * a])
					acc[2 * a] = vlo;
				continue;
			}
			unsigned long long old = acc[2 * a];

			acc[2 * a] += vlo;
			acc[2 * a + 1] += vhi + (acc[2 * a] < old);
		}
	}
	rows_out->clear();
	for (auto &kv : merged)
	{
		rows_out->push_back((unsigned long long) kv.first);
		rows_out->insert(rows_out->end(), kv.second.begin(),
				 kv.second.end());
	}
}

}				/* namespace gg */

#endif /* GG_PLAN_DISTINCT_H */
