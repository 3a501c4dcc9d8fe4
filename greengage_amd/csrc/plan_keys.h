/*
 * The group keys a compiled plan's group code stands for.  ONE definition
 * for every side: plan.cpp decodes every arena row with it, the device top-k
 * (plan_topk.hip) decodes the order's key entries with it, and the
 * COUNT(DISTINCT) regroup (plan_distinct.h) takes the outer key out of an
 * inner code with it, so none of them can drift apart.
 *
 * Plain C++: builds with any C++17 compiler, with or without HIP.
 */
#ifndef GG_PLAN_KEYS_H
#define GG_PLAN_KEYS_H

#include <stdint.h>

#include "plan_dev.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_KEYS_HD __host__ __device__
#else
#define GG_KEYS_HD
#endif

namespace gg
{

/* Group column g of a plan with three or four: columns 0 and 1 are
 * PlanDev's own, columns 2 and 3 the block's (plan_dev.h PlanGroupNDev).  The
 * one place that knows, for the host's ranging, the interpreted kernel and
 * the program generator. */
struct PlanGroupCol
{
	const void *col;
	const uint8_t *nulls;
	int width;
	int src;
};

GG_KEYS_HD static inline PlanGroupCol
plan_group_col(const PlanDev &P, const PlanGroupNDev &N, int g)
{
	if (g < 2)
		return {P.gcol[g], P.gnulls[g], P.gwidth[g], P.pl.gsrc[g]};
	return {N.gcol[g - 2], N.gnulls[g - 2], N.gwidth[g - 2],
		N.gsrc[g - 2]};
}

/* a NULL key is GG_PLAN_NULL_KEY */
GG_KEYS_HD static inline void
plan_keys_of(const PlanGroupPackDev &G, int ngroup, long long code,
	     int64_t *k0, int64_t *k1);

/* The keys of any plan's code: k[0 .. PL_MAX_GCOLS), zero past the plan's
 * columns.  N.n >= 3 is a code of N.n packed fields (plan_dev.h PlanKeysN);
 * every other plan's code is read by (G, ngroup) as ever. */
GG_KEYS_HD static inline void
plan_keys_of(const PlanGroupPackDev &G, const PlanKeysN &N, int ngroup,
	     long long code, int64_t k[PL_MAX_GCOLS])
{
	for (int g = 0; g < PL_MAX_GCOLS; g++)
		k[g] = 0;
	if (N.n < 3)
	{
		plan_keys_of(G, ngroup, code, &k[0], &k[1]);
		return;
	}
	for (int g = 0; g < N.n && g < PL_MAX_GCOLS; g++)
	{
		/* field g lies above shift[g] and below shift[g - 1]; the code
		 * is below 2^62, so field 0 needs no mask */
		uint64_t e = (uint64_t) code >> N.shift[g];

		if (g > 0)
			e &= (1ull << (N.shift[g - 1] - N.shift[g])) - 1;
		k[g] = e ? (int64_t) ((uint64_t) N.gmin[g] + e - 1)
			: GG_PLAN_NULL_KEY;
	}
}

/* the code of G = N.n keys under N, the inverse of the above (has[g] false =
 * NULL); the host's tests and tools encode with it, the scan kernels compute
 * the same expression from their columns */
GG_KEYS_HD static inline long long
plan_code_of(const PlanKeysN &N, const int64_t *k, const bool *has)
{
	uint64_t code = 0;

	for (int g = 0; g < N.n && g < PL_MAX_GCOLS; g++)
		code |= (has[g] ? (uint64_t) k[g] - (uint64_t) N.gmin[g] + 1 : 0)
			<< N.shift[g];
	return (long long) code;
}

GG_KEYS_HD static inline void
plan_keys_of(const PlanGroupPackDev &G, int ngroup, long long code,
	     int64_t *k0, int64_t *k1)
{
	if (G.packed)
	{
		/* (e0 << shift) | e1; e = 0 is NULL, else the
		 * value's offset from the column minimum, plus 1 */
		uint64_t e0 = (uint64_t) code >> G.shift;
		uint64_t e1 = (uint64_t) code & ((1ull << G.shift) - 1);

		*k0 = e0 ? (int64_t) ((uint64_t) G.gmin[0] + e0 - 1)
			: GG_PLAN_NULL_KEY;
		*k1 = e1 ? (int64_t) ((uint64_t) G.gmin[1] + e1 - 1)
			: GG_PLAN_NULL_KEY;
	}
	else if (ngroup == 2)
	{
		long long e0 = code / 512, e1 = code % 512;

		*k0 = e0 == 256 ? GG_PLAN_NULL_KEY : e0;
		*k1 = e1 == 256 ? GG_PLAN_NULL_KEY : e1;
	}
	else
	{
		*k0 = code;
		*k1 = 0;
	}
}

}				/* namespace gg */

#endif /* GG_PLAN_KEYS_H */
